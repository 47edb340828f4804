"""File bytes in, frames out, on the device: JPEG decoding (baseline, and progressive on request) that equals libjpeg's defaults (what
cv2.imread returns) bit for bit.

The stage in front of letterbox.py / augment.py that the reference runs on the host, one file at a time, through cv2.imread
(yolov6/data/datasets.py load_image, LoadData of yolov6/core/inferer.py):
  * parse(data)       host only: walks the markers of one file -> JpegInfo (size, components, tables, restart interval, the scan's byte
                      range, EXIF orientation).  JpegUnsupported names everything outside the supported set, MafError a malformed file;
  * supported(data)   True where decode() takes the file (a caller routes the others to the host decoder);
  * decode(files)     a list of bytes-like objects or paths -> a list of uint8 [h_i, w_i, 3] BGR CUDA tensors: ONE pinned staging buffer, ONE
                      host -> device copy, one chain of launches for the whole call (csrc/jpeg_decode.hip: entropy decode, dequantise +
                      islow IDCT, fancy upsampling + YCbCr -> BGR), no host synchronisation unless check=True reads the status words.
Supported: baseline sequential DCT (SOF0), 8 bit, Huffman, one interleaved scan, 1 component or 3 (Y 1x1, 2x1 or 2x2 with 1x1 chroma).
The pixels follow libjpeg's JDCT_ISLOW + fancy upsampling + jdcolor.c tables as restated in tests/jpeg_ref.py.  cv2.imread also rotates by
the EXIF orientation; by default this decoder does not, so such a file raises JpegUnsupported unless ignore_orientation=True (the stored
pixels).  No CPU fallback.
Opt-in, apply_orientation=True on supported / decode: a file with an EXIF orientation of 2 to 8 decodes into the frame cv2.imread returns,
[h, w, 3] for 2 to 4 and [w, h, 3] for 5 to 8; the orientation travels in the image table and the colour kernel's final store goes through
the permutation (rules restated in tests/jpeg_orientation_ref.py), for baseline and progressive files alike.  A tag value outside 1 to 8
stays refused; together with ignore_orientation it is a MafError.  Without the flag nothing changes.
Opt-in, progressive=True on parse / supported / decode: progressive DCT (SOF2, 8 bit, Huffman) with the same components and samplings, every
scan of the file walked and validated as jdphuff.c start_pass_phuff_decoder does (JpegInfo.scans: one JpegScan per SOS with the Huffman
tables and the restart interval in force there); csrc/jpeg_progressive.hip decodes scan k of every file of the call in launch k, the IDCT
and colour kernels run unchanged on the finished coefficients (rules restated in tests/jpeg_progressive_ref.py).  A progression that leaves
a coefficient unfinished (libjpeg would smooth it) or that libjpeg warns about raises JpegUnsupported.  Without the flag nothing changes.
"""
import struct
from collections import namedtuple
from functools import partial

import numpy as np

from . import lib, staging
from .lib import MafError
from .staging import align as _align, file_bytes as _bytes


class JpegUnsupported(MafError):
    """A well-formed JPEG file outside the supported set (the message names the kind)."""


JpegComponent = namedtuple("JpegComponent", "id h v tq td ta")
JpegInfo = namedtuple("JpegInfo", "width height precision components qtables huffman restart_interval scan orientation adobe_transform scans",
                      defaults=(None,))
JpegScan = namedtuple("JpegScan", "components ss se ah al td ta restart_interval huffman range")
# qtables: {id: uint16 [64] in natural (row-major) order}; huffman: {(class, id): (bits uint8 [16], values uint8 [n])}, class 0 = DC, 1 = AC;
# scan: (first byte, one past the last byte) of the entropy-coded segment, RST markers included; orientation: the EXIF tag or None
# scans: None for a baseline file; for a progressive one (parse(..., progressive=True)) one JpegScan per SOS in file order: components = indices
# into JpegInfo.components, ss / se / ah / al, td / ta = the DC / AC table selector per scan component, and the restart interval, the Huffman
# tables and the byte range of THAT scan (DHT and DRI may change between scans); JpegInfo.scan then spans first scan .. last scan

# jpeg_natural_order of jutils.c: zigzag position -> row-major position
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63],
                  np.int64)

STATUS_BAD_CODE, STATUS_BAD_INDEX, STATUS_SHORT_SCAN, STATUS_REFINE_PAST_SE = 1, 2, 4, 8      # MAF_JPEG_ST_*: bits of a per-image status word
_STATUS_TEXT = ((STATUS_BAD_CODE, "an invalid Huffman code"), (STATUS_BAD_INDEX, "a coefficient index past 63"),
                (STATUS_SHORT_SCAN, "a scan that ends early"), (STATUS_REFINE_PAST_SE, "a refinement run that moves past the end of its band"))

_SOF_NAMES = {0xC1: "extended sequential DCT (SOF1)", 0xC2: "progressive DCT (SOF2)", 0xC3: "lossless (SOF3)",
              0xC5: "differential sequential DCT (SOF5)", 0xC6: "differential progressive DCT (SOF6)", 0xC7: "differential lossless (SOF7)",
              0xC9: "arithmetic coding (SOF9)", 0xCA: "arithmetic coding (SOF10, progressive)", 0xCB: "arithmetic coding (SOF11, lossless)",
              0xCD: "arithmetic coding (SOF13)", 0xCE: "arithmetic coding (SOF14)", 0xCF: "arithmetic coding (SOF15)"}


def _exif_orientation(seg):
    """The orientation tag (0x0112) of IFD0 of an APP1 Exif segment, or None."""
    if len(seg) < 14 or seg[:6] != b"Exif\x00\x00":
        return None
    t = seg[6:]
    if t[:2] == b"II":
        e = "<"
    elif t[:2] == b"MM":
        e = ">"
    else:
        return None
    if struct.unpack(e + "H", t[2:4])[0] != 42:
        return None
    off = struct.unpack(e + "I", t[4:8])[0]
    if off + 2 > len(t):
        return None
    n = struct.unpack(e + "H", t[off:off + 2])[0]
    for i in range(n):
        p = off + 2 + 12 * i
        if p + 12 > len(t):
            return None
        tag, typ, cnt = struct.unpack(e + "HHI", t[p:p + 8])
        if tag == 0x0112 and typ == 3 and cnt == 1:
            return struct.unpack(e + "H", t[p + 8:p + 10])[0]
    return None


def _read_dqt(seg, short, qt):
    """The tables of one DQT segment into qt (natural order)."""
    q = 0
    while q < len(seg):
        pq, tq = seg[q] >> 4, seg[q] & 15
        if pq != 0:
            raise JpegUnsupported("jpeg: 16-bit quantisation tables are not supported")
        if short or q + 65 > len(seg):
            raise MafError("jpeg: a DQT segment runs past the end of the file")
        t = np.zeros(64, np.uint16)
        t[ZIGZAG] = np.frombuffer(seg, np.uint8, 64, q + 1)
        qt[tq] = t
        q += 65


def _read_dht(seg, short, huff):
    """The tables of one DHT segment into huff."""
    q = 0
    if short:
        raise MafError("jpeg: a DHT segment runs past the end of the file")
    while q < len(seg):
        if q + 17 > len(seg):
            raise MafError("jpeg: a DHT segment is cut short")
        tc, th = seg[q] >> 4, seg[q] & 15
        bits = np.frombuffer(seg, np.uint8, 16, q + 1).copy()
        cnt = int(bits.sum())
        if tc > 1 or cnt > 256 or q + 17 + cnt > len(seg):
            raise MafError("jpeg: a malformed DHT segment")
        huff[(tc, th)] = (bits, np.frombuffer(seg, np.uint8, cnt, q + 17).copy())
        q += 17 + cnt


def _check_frame(comps, adobe):
    """The sampling and colour-space limits: 1 component (its factors are irrelevant in a non-interleaved scan) or Y 1x1 / 2x1 / 2x2 with 1x1 chroma."""
    if len(comps) == 3:
        y, cb, cr = comps
        if (cb.h, cb.v, cr.h, cr.v) != (1, 1, 1, 1) or (y.h, y.v) not in ((1, 1), (2, 1), (2, 2)):
            raise JpegUnsupported("jpeg: sampling %s is not supported (Y 1x1, 2x1 or 2x2 with 1x1 chroma)"
                                  % ", ".join("%dx%d" % (c.h, c.v) for c in comps))
        if adobe == 0 or bytes(c.id for c in comps) == b"RGB":
            raise JpegUnsupported("jpeg: an RGB (untransformed) colour space is not supported (YCbCr only)")


def _parse_progressive(d):
    """parse() for a progressive file (SOF2): every scan walked and validated as jdphuff.c start_pass_phuff_decoder does, with libjpeg's
    coef_bits bookkeeping (per component and coefficient: the Al it has reached, -1 = never sent).  What libjpeg only warns about
    (JWRN_BOGUS_PROGRESSION) and a progression that is incomplete at EOI (jdcoefct.c smoothing_ok would smooth) raise JpegUnsupported."""
    n = len(d)
    a = np.frombuffer(d, np.uint8)
    nxt = a[1:]
    # every 0xFF that starts a marker other than RSTn (not a stuffed 0xFF00, not a fill 0xFF): where an entropy-coded segment can end
    marks = np.flatnonzero((a[:-1] == 0xFF) & (nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7)))
    qt, huff = {}, {}
    frame = None
    restart = 0
    orientation = adobe = None
    comps, scans, coef_bits = None, [], None
    p = 2
    while True:
        if p + 2 > n:
            raise MafError("jpeg: the file ends before a scan (no SOS marker)" if not scans else "jpeg: no EOI marker after the scan")
        if d[p] != 0xFF:
            raise MafError("jpeg: expected a marker at byte %d" % p)
        m = d[p + 1]
        if m == 0xFF:
            p += 1
            continue
        p += 2
        if m == 0xD9:
            if not scans:
                raise MafError("jpeg: EOI before any scan")
            break
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if p + 2 > n:
            raise MafError("jpeg: a segment length runs past the end of the file")
        L = (d[p] << 8) | d[p + 1]
        seg = d[p + 2:p + L]
        short = L < 2 or p + L > n
        if m == 0xCC:
            raise JpegUnsupported("jpeg: arithmetic coding (DAC marker) is not supported")
        if m == 0xC0 or m in _SOF_NAMES:
            if frame is not None:
                raise MafError("jpeg: a second SOF marker")
            if m != 0xC2:
                raise MafError("jpeg: a frame header other than the SOF2 the file began with")      # parse() routes here on the first SOF only
            if len(seg) < 6:
                raise MafError("jpeg: the SOF2 segment runs past the end of the file")
            prec, h, w, nf = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8:
                raise JpegUnsupported("jpeg: %d-bit samples are not supported (8-bit only)" % prec)
            if nf not in (1, 3):
                raise JpegUnsupported("jpeg: %d components are not supported (1 or 3)" % nf)
            if short or len(seg) < 6 + 3 * nf:
                raise MafError("jpeg: the SOF2 segment runs past the end of the file")
            if h == 0 or w == 0:
                raise JpegUnsupported("jpeg: a frame height of 0 (DNL marker) is not supported" if w else "jpeg: zero width")
            frame = (w, h)
            comps = tuple(JpegComponent(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i], 0, 0) for i in range(nf))
            _check_frame(comps, None)
            coef_bits = [[-1] * 64 for _ in comps]
        elif m == 0xDB:
            if scans:
                raise JpegUnsupported("jpeg: a DQT segment after the first SOS of a progressive file is not supported")
            _read_dqt(seg, short, qt)
        elif m == 0xC4:
            _read_dht(seg, short, huff)
        elif m == 0xDD:
            if short or len(seg) < 2:
                raise MafError("jpeg: the DRI segment runs past the end of the file")
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xDC:
            raise JpegUnsupported("jpeg: a DNL marker is not supported")
        elif m == 0xE1:
            if short:
                raise MafError("jpeg: an APP1 segment runs past the end of the file")
            o = _exif_orientation(seg)
            orientation = o if o is not None else orientation
        elif m == 0xEE:
            if short:
                raise MafError("jpeg: an APP14 segment runs past the end of the file")
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            k = len(scans)
            if frame is None:
                raise MafError("jpeg: SOS before SOF")
            if len(seg) < 1:
                raise MafError("jpeg: the SOS segment runs past the end of the file")
            ns = seg[0]
            if ns < 1 or ns > 4:
                raise MafError("jpeg: scan %d names %d components" % (k, ns))
            if short or len(seg) < 4 + 2 * ns:
                raise MafError("jpeg: the SOS segment runs past the end of the file")
            ids = [c.id for c in comps]
            idx, td, ta = [], [], []
            for i in range(ns):
                if seg[1 + 2 * i] not in ids:
                    raise MafError("jpeg: scan %d names component id %d, which the frame does not have" % (k, seg[1 + 2 * i]))
                idx.append(ids.index(seg[1 + 2 * i]))
                td.append(seg[2 + 2 * i] >> 4)
                ta.append(seg[2 + 2 * i] & 15)
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            what = "scan %d (components %s, Ss %d, Se %d, Ah %d, Al %d)" % (k, idx, ss, se, ah, al)
            # jdphuff.c start_pass_phuff_decoder (JERR_BAD_PROGRESSION there)
            if ss == 0:
                if se != 0:
                    raise JpegUnsupported("jpeg: %s: a progressive scan that starts at the DC coefficient must end there (Ss 0 needs Se 0)" % what)
            elif ns != 1:
                raise JpegUnsupported("jpeg: %s: a progressive AC scan takes one component" % what)
            elif se < ss or se > 63:
                raise JpegUnsupported("jpeg: %s: a progressive AC band needs Ss <= Se <= 63" % what)
            if ah != 0 and al != ah - 1:
                raise JpegUnsupported("jpeg: %s: a progressive refinement scan needs Al = Ah - 1" % what)
            if al > 13:
                raise JpegUnsupported("jpeg: %s: a progressive scan with Al above 13" % what)
            if ns > 1 and idx != list(range(len(comps))):
                raise JpegUnsupported("jpeg: %s: a progressive DC scan of some of the components, or in another order, is not supported "
                                      "(all of them in frame order, or one)" % what)
            for j, c in enumerate(idx):                     # the coef_bits loop (JWRN_BOGUS_PROGRESSION there)
                bits = coef_bits[c]
                if ss != 0 and bits[0] < 0:
                    raise JpegUnsupported("jpeg: %s: a bogus progression, an AC scan before the component's first DC scan" % what)
                for ci in range(ss, se + 1):
                    if ah != max(bits[ci], 0):
                        raise JpegUnsupported("jpeg: %s: a bogus progression, Ah %d where coefficient %d stands at %s" %
                                              (what, ah, ci, "bit %d" % bits[ci] if bits[ci] >= 0 else "never sent"))
                    bits[ci] = al
                sel = td[j] if ss == 0 else ta[j]
                if ss == 0 and ah != 0:
                    continue                                # a DC refinement scan reads raw bits: no table
                if sel > 1:
                    raise JpegUnsupported("jpeg: Huffman table selectors above 1 are not supported")
                if (0 if ss == 0 else 1, sel) not in huff:
                    raise MafError("jpeg: Huffman table %s %d of scan %d is missing" % ("DC" if ss == 0 else "AC", sel, k))
            p += L
            at = int(np.searchsorted(marks, p))
            if at >= marks.size:
                raise MafError("jpeg: no EOI marker after the scan")
            end = int(marks[at])
            scans.append(JpegScan(tuple(idx), ss, se, ah, al, tuple(td), tuple(ta), restart, dict(huff), (p, end)))
            p = end
            continue
        elif short:
            raise MafError("jpeg: a segment (marker 0xFF%02X) runs past the end of the file" % m)
        p += L
    _check_frame(comps, adobe)
    for c in comps:
        if c.tq not in qt:
            raise MafError("jpeg: quantisation table %d is missing" % c.tq)
    for c, bits in enumerate(coef_bits):
        left = [ci for ci in range(64) if bits[ci] != 0]
        if left:
            raise JpegUnsupported("jpeg: an incomplete progression is not supported (libjpeg would smooth the blocks): after the %d scans of the "
                                  "file, coefficient %d of component %d %s" % (len(scans), left[0], c, "was never sent" if bits[left[0]] < 0
                                                                               else "stands at bit %d" % bits[left[0]]))
    return JpegInfo(frame[0], frame[1], 8, comps, qt, dict(huff), scans[0].restart_interval, (scans[0].range[0], scans[-1].range[1]), orientation,
                    adobe, tuple(scans))


def parse(data, progressive=False):
    """Walk the markers of one JPEG file (bytes-like or a path) -> JpegInfo.  Host only.  progressive=True also takes SOF2 files (JpegInfo.scans)."""
    d = _bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise MafError("jpeg: no SOI marker at the start (not a JPEG file)")
    qt, huff = {}, {}
    frame = None
    restart = 0
    orientation = None
    adobe = None
    p = 2
    while True:
        if p + 2 > n:
            raise MafError("jpeg: the file ends before a scan (no SOS marker)")
        if d[p] != 0xFF:
            raise MafError("jpeg: expected a marker at byte %d" % p)
        m = d[p + 1]
        if m == 0xFF:                                       # fill byte
            p += 1
            continue
        p += 2
        if m == 0xD9:
            raise MafError("jpeg: EOI before any scan")
        if m == 0x01 or 0xD0 <= m <= 0xD7:                  # stand-alone markers
            continue
        if p + 2 > n:
            raise MafError("jpeg: a segment length runs past the end of the file")
        L = (d[p] << 8) | d[p + 1]
        seg = d[p + 2:p + L]
        short = L < 2 or p + L > n                          # judged after the fields that name an unsupported kind have been read
        if m == 0xCC:
            raise JpegUnsupported("jpeg: arithmetic coding (DAC marker) is not supported")
        if m == 0xC2 and progressive and frame is None:
            return _parse_progressive(d)
        if m in _SOF_NAMES:
            raise JpegUnsupported("jpeg: %s is not supported (baseline SOF0 only)" % _SOF_NAMES[m] if not progressive else
                                  "jpeg: %s is not supported (baseline SOF0 and progressive SOF2 only)" % _SOF_NAMES[m])
        if m == 0xC0:
            if len(seg) < 6:
                raise MafError("jpeg: the SOF0 segment runs past the end of the file")
            prec, h, w, nf = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8:
                raise JpegUnsupported("jpeg: %d-bit samples are not supported (8-bit only)" % prec)
            if nf not in (1, 3):
                raise JpegUnsupported("jpeg: %d components are not supported (1 or 3)" % nf)
            if short or len(seg) < 6 + 3 * nf:
                raise MafError("jpeg: the SOF0 segment runs past the end of the file")
            if frame is not None:
                raise MafError("jpeg: a second SOF marker")
            if h == 0 or w == 0:
                raise JpegUnsupported("jpeg: a frame height of 0 (DNL marker) is not supported" if w else "jpeg: zero width")
            frame = (w, h, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)])
        elif m == 0xDB:
            _read_dqt(seg, short, qt)
        elif m == 0xC4:
            _read_dht(seg, short, huff)
        elif m == 0xDD:
            if short or len(seg) < 2:
                raise MafError("jpeg: the DRI segment runs past the end of the file")
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xE1:
            if short:
                raise MafError("jpeg: an APP1 segment runs past the end of the file")
            o = _exif_orientation(seg)
            orientation = o if o is not None else orientation
        elif m == 0xEE:
            if short:
                raise MafError("jpeg: an APP14 segment runs past the end of the file")
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise MafError("jpeg: SOS before SOF")
            if len(seg) < 1:
                raise MafError("jpeg: the SOS segment runs past the end of the file")
            ns = seg[0]
            if ns != len(frame[2]):
                raise JpegUnsupported("jpeg: more than one scan (a scan of %d of the %d components) is not supported" % (ns, len(frame[2])))
            if short or len(seg) < 4 + 2 * ns:
                raise MafError("jpeg: the SOS segment runs past the end of the file")
            comps = []
            for i, (cid, ch, cv, tq) in enumerate(frame[2]):
                if seg[1 + 2 * i] != cid:
                    raise JpegUnsupported("jpeg: a scan whose component order differs from the frame's is not supported")
                comps.append(JpegComponent(cid, ch, cv, tq, seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15))
            ss, se, a = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]
            if (ss, se, a) != (0, 63, 0):
                raise JpegUnsupported("jpeg: a scan with spectral selection or successive approximation (progressive) is not supported")
            p += L
            break
        elif short:
            raise MafError("jpeg: a segment (marker 0xFF%02X) runs past the end of the file" % m)
        p += L
    w, h, _ = frame
    _check_frame(comps, adobe)
    for c in comps:
        if c.tq not in qt:
            raise MafError("jpeg: quantisation table %d is missing" % c.tq)
        if c.td > 1 or c.ta > 1:
            raise JpegUnsupported("jpeg: Huffman table selectors above 1 (not baseline) are not supported")
        if (0, c.td) not in huff or (1, c.ta) not in huff:
            raise MafError("jpeg: Huffman table DC %d / AC %d is missing" % (c.td, c.ta))
    # the entropy-coded segment ends at the first marker that is neither a stuffed 0xFF00 nor RSTn (nor a fill 0xFF)
    a = np.frombuffer(d, np.uint8, n - p, p)
    nxt = a[1:]
    hit = np.flatnonzero((a[:-1] == 0xFF) & (nxt != 0) & (nxt != 0xFF) & ((nxt < 0xD0) | (nxt > 0xD7)))
    if hit.size == 0:
        raise MafError("jpeg: no EOI marker after the scan")
    end = p + int(hit[0])
    m = d[end + 1]
    if m == 0xDA or m == 0xC4 or m == 0xDB or m == 0xDD:
        raise JpegUnsupported("jpeg: more than one scan is not supported")
    if m == 0xDC:
        raise JpegUnsupported("jpeg: a DNL marker is not supported")
    if m != 0xD9:
        raise MafError("jpeg: marker 0xFF%02X after the scan where EOI should be" % m)
    return JpegInfo(w, h, 8, tuple(comps), qt, huff, restart, (p, end), orientation, adobe)


def supported(data, progressive=False, apply_orientation=False):
    """True where decode() takes this file: a baseline JPEG (with progressive=True also a progressive one) of the supported set without an
    EXIF rotation; with apply_orientation=True also one with an EXIF orientation of 2 to 8."""
    try:
        return parse(data, progressive).orientation in ((None,) + tuple(range(1, 9)) if apply_orientation else (None, 1))
    except MafError:
        return False


# ---------------------------------------------------------------- device tables (host side)

HUFF_LOOK_BITS = 9            # MAF_JPEG_LOOK_BITS: codes up to this length resolve in one table read
HUFF_TABLE_BYTES = 2 * (1 << HUFF_LOOK_BITS) + 4 * 18 + 4 * 18 + 256      # look u16 [512] | maxcode i32 [18] | valoff i32 [18] | huffval u8 [256]
HUFF_SET_BYTES = 4 * HUFF_TABLE_BYTES                                     # DC 0, DC 1, AC 0, AC 1
MAX_GROUP = 64                # MAF_JPEG_GROUP: the most decoding lanes of one workgroup (one wave); they share one set of Huffman tables
WAVE_SLOTS = 2048             # 256 CUs x 8: while the chip has free slots a wave carries one lane (the lanes of a wave diverge and serialise)

IMAGE_DT = np.dtype([("coef_off", "<i8"), ("plane_off", "<i8"), ("out_off", "<i8"), ("w", "<i4"), ("h", "<i4"), ("ncomp", "<i4"), ("hs", "<i4"),
                     ("vs", "<i4"), ("mcux", "<i4"), ("mcuy", "<i4"), ("quant", "<i4"), ("dc_tab", "<i4", 3), ("ac_tab", "<i4", 3),
                     ("orientation", "<i4"), ("reserved", "<i4")])   # maf_jpeg_image_t
LANE_DT = np.dtype([("begin", "<i8"), ("end", "<i8"), ("image", "<i4"), ("first_mcu", "<i4"), ("n_mcu", "<i4"), ("tabset", "<i4")])   # maf_jpeg_lane_t
HEADER_DT = np.dtype([("n_images", "<i4"), ("n_lanes", "<i4"), ("n_tabsets", "<i4"), ("group", "<i4"), ("images_off", "<i8"), ("lanes_off", "<i8"),
                      ("huff_off", "<i8"), ("quant_off", "<i8"), ("scan_off", "<i8"), ("scan_bytes", "<i8"), ("total_bytes", "<i8"),
                      ("coef_elems", "<i8"), ("plane_bytes", "<i8"), ("out_bytes", "<i8"), ("n_scans", "<i4"), ("n_slanes", "<i4"), ("n_rounds", "<i4"),
                      ("sgroup", "<i4"), ("scans_off", "<i8"), ("slanes_off", "<i8"), ("rounds_off", "<i8")])  # maf_jpeg_header_t
SCAN_DT = np.dtype([("image", "<i4"), ("round", "<i4"), ("ncomp", "<i4"), ("comp", "<i4", 3), ("ss", "<i4"), ("se", "<i4"), ("ah", "<i4"), ("al", "<i4"),
                    ("dc_tab", "<i4", 3), ("ac_tab", "<i4"), ("bw", "<i4"), ("bh", "<i4")])               # maf_jpeg_scan_t
SCAN_PAD = 64                 # zero bytes the host appends to the scan buffer (the bit reader's clamp lands in them)
STAGE_ENTROPY, STAGE_IDCT, STAGE_COLOR, STAGE_ALL = 1, 2, 4, 7


def huff_device_table(bits, vals):
    """One Huffman table in the layout the entropy kernel keeps in LDS (jpeg_make_d_derived_tbl of jdhuff.c, with a 9-bit lookahead):
    look[c] = length << 8 | symbol for every 9-bit prefix c that starts with a code of at most 9 bits, else 0; for longer codes
    maxcode[l] (-1: no code of length l) and valoff[l] with symbol = huffval[valoff[l] + code]."""
    out = np.zeros(HUFF_TABLE_BYTES, np.uint8)
    look = out[:1024].view("<u2")
    maxcode = out[1024:1096].view("<i4")
    valoff = out[1096:1168].view("<i4")
    out[1168:1168 + len(vals)] = vals
    maxcode[:] = -1
    code, k = 0, 0
    for l in range(1, 17):
        nl = int(bits[l - 1])
        if nl:
            if code + nl > (1 << l):
                raise MafError("jpeg: a Huffman table assigns more codes than its lengths allow")
            valoff[l] = k - code
            if l <= HUFF_LOOK_BITS:
                for i in range(nl):
                    c = (code + i) << (HUFF_LOOK_BITS - l)
                    look[c:c + (1 << (HUFF_LOOK_BITS - l))] = (l << 8) | int(vals[k + i])
            code += nl
            k += nl
            maxcode[l] = code - 1
        code <<= 1
    maxcode[17] = 0xFFFFF                                   # jdhuff.c's sentinel: ends the search
    return out


def _restart_ranges(d, scan, n_lanes):
    """Byte ranges of the restart intervals inside the scan (RST markers excluded) -> [(begin, end)] * n_lanes; intervals the scan does
    not hold come back empty (the device reports them as a scan that ends early)."""
    s, e = scan
    if n_lanes == 1:
        return [(s, e)]
    a = np.frombuffer(d, np.uint8, e - s, s)
    nxt = a[1:]
    at = (np.flatnonzero((a[:-1] == 0xFF) & (nxt >= 0xD0) & (nxt <= 0xD7)) + s).tolist()[:n_lanes - 1]
    begins = [s] + [x + 2 for x in at]
    ends = at + [e]
    out = list(zip(begins, ends))
    return out + [(e, e)] * (n_lanes - len(out))


def geometry(info):
    """(ncomp, hs, vs, mcux, mcuy, blocks per component) of a parsed file."""
    nc = len(info.components)
    hs, vs = (info.components[0].h, info.components[0].v) if nc == 3 else (1, 1)
    mcux, mcuy = -(-info.width // (8 * hs)), -(-info.height // (8 * vs))
    blocks = [mcux * hs * mcuy * vs] + [mcux * mcuy] * (nc - 1)
    return nc, hs, vs, mcux, mcuy, blocks


def scan_geometry(info, scan):
    """(blocks per row, block rows) of the MCU grid of one scan of a progressive file: the frame's MCU grid for the interleaved (DC) scan of
    all components; for a one-component scan ceil(comp_w / 8) x ceil(comp_h / 8) blocks over the component's OWN sample dimensions (an MCU is
    one block there: jdinput.c per_scan_setup), which is smaller than the padded grid the coefficient buffer is addressed by."""
    nc, hs, vs, mcux, mcuy, _ = geometry(info)
    if len(scan.components) > 1:
        return mcux, mcuy
    ch, cv = (hs, vs) if scan.components[0] == 0 else (1, 1)
    cw, chh = -(-info.width * ch // hs), -(-info.height * cv // vs)
    return -(-cw // 8), -(-chh // 8)


def _group_of(n_lanes):
    """Lanes per one-wave workgroup: 1 while the chip has free wave slots, doubling (up to MAX_GROUP) beyond."""
    group = 1
    while group < MAX_GROUP and n_lanes > WAVE_SLOTS * group:
        group *= 2
    return group


def build_blob(datas, infos, apply_orientation=False):
    """Everything the device needs for one call, in one byte array: header | image table | lane table | Huffman table sets | quantisation
    tables | with progressive files: scan table | scan lanes | round starts | the scans' bytes + SCAN_PAD zeros.
    -> (header record, image table, lane table, Huffman table sets, quantisation tables, each file's offset in the scan bytes,
    (scan table, scan lanes, round starts) or None).  apply_orientation: the image table carries each file's EXIF orientation (else 0: the
    stored grid)."""
    B = len(infos)
    images = np.zeros(B, IMAGE_DT)
    quant = np.zeros((B, 3, 64), np.uint16)
    tabsets, set_bytes, groups = {}, [], []
    coef = plane = outb = scanb = 0
    scan_at = []
    scan_rows, rounds = [], []             # progressive files: the scan table; rounds[k][table set] = lanes of the k-th scan of every file that has one

    def tabset_of(key):
        if key not in tabsets:
            tabsets[key] = len(set_bytes)
            set_bytes.append(np.concatenate([np.zeros(HUFF_TABLE_BYTES, np.uint8) if t is None else
                                             huff_device_table(np.frombuffer(t[0], np.uint8), np.frombuffer(t[1], np.uint8)) for t in key]))
            groups.append([])
        return tabsets[key]

    for i, (d, info) in enumerate(zip(datas, infos)):
        nc, hs, vs, mcux, mcuy, blocks = geometry(info)
        im = images[i]
        im["coef_off"], im["plane_off"], im["out_off"] = coef, plane, outb
        im["w"], im["h"], im["ncomp"], im["hs"], im["vs"], im["mcux"], im["mcuy"], im["quant"] = info.width, info.height, nc, hs, vs, mcux, mcuy, 3 * i
        if apply_orientation and info.orientation is not None:
            im["orientation"] = info.orientation
        for c, comp in enumerate(info.components):
            quant[i, c] = info.qtables[comp.tq]
            im["dc_tab"][c], im["ac_tab"][c] = comp.td, comp.ta
        coef += 64 * sum(blocks)
        plane += 64 * sum(blocks)
        outb += _align(3 * info.width * info.height)
        s, e = info.scan
        if info.scans is not None:                           # progressive: one scan-table row and one lane per restart interval of every scan
            for k, sc in enumerate(info.scans):
                dc = sc.ss == 0
                used = set() if dc and sc.ah else {(0 if dc else 1, t) for t in (sc.td if dc else sc.ta)}
                ts = tabset_of(tuple((sc.huffman[q][0].tobytes(), sc.huffman[q][1].tobytes()) if q in used else None
                                     for q in ((0, 0), (0, 1), (1, 0), (1, 1))))
                bw, bh = scan_geometry(info, sc)
                total = bw * bh
                ri = sc.restart_interval if sc.restart_interval else total
                nl = -(-total // ri)
                while len(rounds) <= k:
                    rounds.append({})
                row = rounds[k].setdefault(ts, [])
                for j, (b0, b1) in enumerate(_restart_ranges(d, sc.range, nl)):
                    row.append((scanb + b0 - s, scanb + b1 - s, len(scan_rows), j * ri, min(ri, total - j * ri), ts))
                scan_rows.append((i, k, len(sc.components), tuple(sc.components) + (0,) * (3 - len(sc.components)), sc.ss, sc.se, sc.ah, sc.al,
                                  tuple(sc.td) + (0,) * (3 - len(sc.td)) if dc else (0, 0, 0), 0 if dc else sc.ta[0], bw, bh))
            scan_at.append(scanb)
            scanb += e - s
            continue
        ts = tabset_of(tuple(None if k not in info.huffman else (info.huffman[k][0].tobytes(), info.huffman[k][1].tobytes())
                             for k in ((0, 0), (0, 1), (1, 0), (1, 1))))
        total = mcux * mcuy
        ri = info.restart_interval if info.restart_interval else total
        nl = -(-total // ri)
        for k, (b0, b1) in enumerate(_restart_ranges(d, info.scan, nl)):
            groups[ts].append((scanb + b0 - s, scanb + b1 - s, i, k * ri, min(ri, total - k * ri), ts))
        scan_at.append(scanb)
        scanb += e - s
    rows, group = [], _group_of(sum(len(g) for g in groups))
    for ts, g in enumerate(groups):                          # lanes of one workgroup share a table set: pad every set's lanes to whole groups
        rows += g + [(0, 0, -1, 0, 0, ts)] * (-len(g) % group)
    lanes = np.array(rows, LANE_DT)
    srows, starts = [], [0]                                  # the scan lanes, round after round, each round's table sets padded to whole groups
    sgroup = _group_of(max((sum(len(g) for g in r.values()) for r in rounds), default=0))
    for r in rounds:
        for ts, g in r.items():
            srows += g + [(0, 0, -1, 0, 0, ts)] * (-len(g) % sgroup)
        starts.append(len(srows))
    huff = np.concatenate(set_bytes)
    prog = (np.array(scan_rows, SCAN_DT), np.array(srows, LANE_DT), np.array(starts, np.int32)) if scan_rows else None
    hdr, off = staging.blob_layout(HEADER_DT, _sections(images, lanes, huff, quant, prog))
    hdr["n_images"], hdr["n_lanes"], hdr["n_tabsets"], hdr["group"] = B, len(lanes), len(set_bytes), group
    if prog is not None:                                     # a call without progressive files has none of these sections
        hdr["n_scans"], hdr["n_slanes"], hdr["n_rounds"], hdr["sgroup"] = len(prog[0]), len(prog[1]), len(rounds), sgroup
    hdr["scan_off"] = off
    hdr["scan_bytes"] = _align(scanb + SCAN_PAD)           # a multiple of 8: the bit reader loads aligned 8-byte words
    hdr["total_bytes"] = off + _align(scanb + SCAN_PAD)
    hdr["coef_elems"], hdr["plane_bytes"], hdr["out_bytes"] = coef, plane, outb
    if hdr["total_bytes"] >= staging.MAX_BLOB or B > staging.MAX_FILES:
        raise MafError("jpeg: decode() takes up to 65535 files and 2 GiB of file bytes per call")
    return hdr, images, lanes, huff, quant, scan_at, prog


def _sections(images, lanes, huff, quant, prog):
    """The sections in front of the scan bytes, by header field, in blob order."""
    return [("images_off", images), ("lanes_off", lanes), ("huff_off", huff), ("quant_off", quant)] + \
        (list(zip(("scans_off", "slanes_off", "rounds_off"), prog)) if prog is not None else [])


def fill_blob(buf, hdr, images, lanes, huff, quant, datas, infos, scan_at, prog=None):
    """Write the sections of build_blob into `buf` (a uint8 array of hdr.total_bytes: the pinned staging buffer)."""
    staging.write_blob(buf, hdr, _sections(images, lanes, huff, quant, prog))
    so = int(hdr["scan_off"])
    for d, info, at in zip(datas, infos, scan_at):
        s, e = info.scan
        buf[so + at:so + at + e - s] = np.frombuffer(d, np.uint8, e - s, s)
    buf[so + (scan_at[-1] + infos[-1].scan[1] - infos[-1].scan[0] if infos else 0):] = 0      # at least SCAN_PAD zero bytes


_library = partial(staging.checked_library, "jpeg", (("maf_jpeg_struct_sizes", 3), ("maf_jpeg_progressive_struct_sizes", 1)),
                   [HEADER_DT.itemsize, IMAGE_DT.itemsize, LANE_DT.itemsize, SCAN_DT.itemsize], "maf_jpeg_* structs")
status_text = partial(staging.status_text, _STATUS_TEXT)


def decode(files, device=None, stream=None, ignore_orientation=False, check=True, stages=STAGE_ALL, taps=None, progressive=False,
           apply_orientation=False):
    """Decode a list of baseline JPEG files (bytes-like objects or paths; mixed sizes and samplings welcome) on the device; with
    progressive=True the list may also hold progressive files (scan k of every file of the call is one launch: jpeg_prog_entropy_kernel).
    -> a list of uint8 [h_i, w_i, 3] BGR CUDA tensors (views of one allocation), what cv2.imread returns for each file; they go into
    letterbox / eval_batch / detect_frames / train_batch as they are.  With check=True (the default) the per-image status words are read
    once after the launches (the call's one synchronisation) and a fault raises MafError naming the file; check=False returns
    (frames, status int32 [B]) without synchronising.  `stream`: a torch.cuda.Stream to work on (default: the current one).
    apply_orientation=True: a file with an EXIF orientation of 2 to 8 decodes into the frame cv2.imread returns, [h, w, 3] for 2 to 4 and
    [w, h, 3] for 5 to 8 (the colour kernel's final store goes through the permutation: no further launch or buffer); a tag value outside
    1 to 8 stays refused.  Not together with ignore_orientation.
    `taps`: a dict that receives the intermediate buffers (coefficients, planes, the image table with h and w as the frames have them;
    "progressive": the scan table, the scan lanes and the round starts, or None) — tests and the probe."""
    extra = {}
    if apply_orientation and ignore_orientation:
        raise MafError("jpeg.decode: apply_orientation and ignore_orientation exclude each other (rotate the frame, or take the stored pixels)")

    def parse_one(d):
        info = parse(d, progressive)
        if apply_orientation:
            if info.orientation is not None and not 1 <= info.orientation <= 8:
                raise JpegUnsupported("jpeg: EXIF orientation %d is not one of 1 to 8" % info.orientation)
        elif info.orientation not in (None, 1) and not ignore_orientation:
            raise JpegUnsupported("jpeg: EXIF orientation %d — cv2.imread would rotate the frame, this decoder does not "
                                  "(pass ignore_orientation=True to take the stored pixels)" % info.orientation)
        return info

    def build(datas, infos):
        hdr, images, lanes, huff, quant, scan_at, prog = build_blob(datas, infos, apply_orientation)
        extra["progressive"] = prog
        shown = images
        if (images["orientation"] >= 5).any():                   # the frames of orientations 5 to 8 are [w, h, 3]: the views' table, not the blob's
            shown = images.copy()
            turned = shown["orientation"] >= 5
            shown["h"][turned], shown["w"][turned] = images["w"][turned], images["h"][turned]
        return hdr, shown, lambda host: fill_blob(host, hdr, images, lanes, huff, quant, datas, infos, scan_at, prog)

    def launch(L, s, blob, hdr, out, status):
        import torch
        coef = torch.empty(int(hdr["coef_elems"]), dtype=torch.int16, device=s.dev)
        planes = torch.empty(int(hdr["plane_bytes"]), dtype=torch.uint8, device=s.dev)
        lib.check(L.maf_jpeg_decode(s.host.ctypes.data, blob.data_ptr(), coef.data_ptr(), planes.data_ptr(), out.data_ptr(), status.data_ptr(),
                                    int(stages), s.stream.cuda_stream))
        return dict(extra, coef=coef, planes=planes)

    return staging.decode_files("jpeg.decode", files, parse_one, build, _library, launch, _STATUS_TEXT, False, device, stream, check, taps)
