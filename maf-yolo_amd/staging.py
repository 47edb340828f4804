"""The staging scaffold the image codecs and resizers share (jpeg.py, png.py, jpeg_encode.py, letterbox.py, frames.py, augment.py): a new one
starts here and in csrc/image_blob.h.

What a call of theirs does around its kernels, each piece once:
  * checked_library       the HIP library, with the caller's struct sizes compared against it on the first call (lib.check_sizes);
  * blob_layout / write_blob   the blob idiom: a header record, then sections at 16-byte-aligned offsets the header names;
  * staged                the staging discipline: the work runs on one device and stream, the blob travels in ONE pinned buffer with ONE
                          non_blocking host -> device copy, and the pinned buffer lives until the block ends;
  * decode_files          the body of jpeg.decode and png.decode (parse every file, stage, launch, frame views, status words);
  * frame_list            the checks of a list of uint8 [h, w, 3] CUDA frames, worded by the caller;
  * rect_list             the rectangles of those frames an encoder writes one file each for, checked;
  * file_bytes, file_name, status_text, frame_views, raise_on_status, cuda_device, upload, align: the small change.
A leaf: it imports lib and numpy only, torch where a function needs the device.
"""
import contextlib
import ctypes
import os
import types

import numpy as np

from . import lib
from .lib import MafError

MAX_FILES = 65535             # files (images, jobs) of one call: the blob entry points' limit
MAX_BLOB = 2 ** 31            # bytes of one blob, exclusive


def align(x, a=16):
    return (x + a - 1) // a * a


_checked = set()


def checked_library(key, size_fns, want, what):
    """lib.load(), with the struct sizes of a binding checked against the library on the first call per `key`.  size_fns: ((name of a
    maf_*_struct_sizes export, how many int32 it fills), ...); want: the sizes this binding declares, in that order (a list; a bare int
    where one export fills one size); what: the structs' name in the MafError a mismatch raises."""
    L = lib.load()
    if key not in _checked:
        have = []
        for name, n in size_fns:
            sizes = (ctypes.c_int32 * n)()
            lib.check(getattr(L, name)(sizes))
            have += list(sizes)
        lib.check_sizes(what, have if isinstance(want, list) else have[0], want)
        _checked.add(key)
    return L


def blob_layout(header_dt, sections):
    """The layout of a blob: the header record, then every (header field, array) of `sections` in order, each at a 16-byte-aligned offset
    that is written into its header field -> (header record, zero but for the offsets; the aligned end of the last section)."""
    hdr = np.zeros(1, header_dt)[0]
    off = align(header_dt.itemsize)
    for name, arr in sections:
        hdr[name] = off
        off = align(off + arr.nbytes)
    return hdr, off


def write_blob(buf, hdr, sections):
    """Write the header record and the sections of blob_layout into `buf` (uint8)."""
    buf[:hdr.dtype.itemsize] = np.frombuffer(hdr.tobytes(), np.uint8)
    for name, arr in sections:
        o = int(hdr[name])
        buf[o:o + arr.nbytes] = arr.reshape(-1).view(np.uint8)


@contextlib.contextmanager
def staged(nbytes, dev, stream=None, zeros=False):
    """with staged(nbytes, dev, stream) as s: the block runs on `dev` and on s.stream (`stream`, default: the device's current one);
    s.pinned is a pinned uint8 tensor of nbytes (zeros=True: zeroed) and s.host its numpy view, for the caller to fill; s.copy() is the
    call's one host -> device copy.  `s` holds the pinned buffer, so it lives as long as the block does."""
    import torch
    st = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.device(dev), torch.cuda.stream(st):
        pinned = (torch.zeros if zeros else torch.empty)(nbytes, dtype=torch.uint8, pin_memory=True)
        yield types.SimpleNamespace(dev=dev, stream=st, pinned=pinned, host=pinned.numpy(), copy=lambda: pinned.to(dev, non_blocking=True))


def upload(arr, dev):
    """Host array -> device on the current stream, without a host sync (pinned staging)."""
    import torch
    return torch.from_numpy(arr).pin_memory().to(dev, non_blocking=True)


def cuda_device(device, what):
    """`device` (None: the current CUDA device) as a torch.device with an index; anything but a CUDA device raises."""
    import torch
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise MafError("%s runs on the HIP path only (no CPU fallback): device %s" % (what, dev))
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def file_bytes(data):
    """The bytes of a file given as a path, or of a bytes-like object."""
    if isinstance(data, (str, os.PathLike)):
        with open(data, "rb") as f:
            return f.read()
    return bytes(data)


def file_name(f, i):
    return "file %d (%s)" % (i, os.fspath(f)) if isinstance(f, (str, os.PathLike)) else "file %d" % i


def status_text(table, word):
    """The set bits of a status word in the words of `table` ((bit, text), ...)."""
    return ", ".join(t for bit, t in table if word & bit) or "status 0x%x" % word


def frame_views(out, images):
    """The frames of an image table (out_off, h, w per image) as uint8 [h, w, 3] views of `out`."""
    frames = []
    for im in images:
        o, h, w = int(im["out_off"]), int(im["h"]), int(im["w"])
        frames.append(out[o:o + 3 * h * w].view(h, w, 3))
    return frames


def raise_on_status(what, files, words, table, with_hex):
    """MafError naming every file whose status word is not 0 (with_hex: the word itself behind its text)."""
    bad = [(i, w) for i, w in enumerate(words) if w]
    if bad:
        raise MafError("%s: " % what + "; ".join("%s: %s" % (file_name(files[i], i), status_text(table, w)) + (" (status 0x%x)" % w if with_hex else "")
                                                 for i, w in bad))


def decode_files(what, files, parse_one, build, library, launch, table, with_hex, device=None, stream=None, check=True, taps=None):
    """The body of a decode(files) call `what`.  The caller's hooks, in the order they run:
      parse_one(bytes) -> info             a MafError of it is raised again with the file's name in front;
      build(datas, infos) -> (hdr, images, fill)   the blob's header record (total_bytes, out_bytes), the image table (out_off, h, w) and
                                           fill(host) that writes the blob into the pinned buffer;
      library() -> the HIP library;
      launch(L, s, blob, hdr, out, status) -> dict   the scratch allocations and the entry point, on s.stream (s: the `staged` block);
                                           the dict goes into `taps` beside images, status and header.
    -> the frames; with check=False (frames, status) without synchronising."""
    import torch
    files = list(files)
    if not files:
        raise MafError("%s: no files" % what)
    dev = cuda_device(device, what)
    datas, infos = [], []
    for i, f in enumerate(files):
        d = file_bytes(f)
        try:
            infos.append(parse_one(d))
        except MafError as e:
            raise type(e)("%s: %s" % (file_name(f, i), e)) from None
        datas.append(d)
    hdr, images, fill = build(datas, infos)
    L = library()
    with staged(int(hdr["total_bytes"]), dev, stream) as s:
        fill(s.host)
        blob = s.copy()
        out = torch.empty(int(hdr["out_bytes"]), dtype=torch.uint8, device=dev)
        status = torch.empty(len(files), dtype=torch.int32, device=dev)
        extra = launch(L, s, blob, hdr, out, status)
        frames = frame_views(out, images)
        if taps is not None:
            taps.update(extra, images=images, status=status, header=hdr)
        if not check:
            return frames, status
        words = status.tolist()                                                  # the one synchronisation (the pinned buffer is alive until the copy is done)
    raise_on_status(what, files, words, table, with_hex)
    return frames


def frame_list(frames, text, what=None):
    """A list of uint8 [h, w, 3] CUDA frames with pixel stride 3 and channel stride 1, or one [B, h, w, 3] tensor -> the list, checked.
    text: the caller's wording, a %-format per check in the order they run: "batch" (shape), "none", per frame i "not_tensor" (kind), "cpu"
    (device), "type" (dtype, shape), "stride" (strides), and the checks made only where the caller words them: "device" (all frames on
    frame 0's), "empty" and "too_large" (w, h: a side of 0 or above 65535) in front of "stride", "pitch" (a row pitch below 3 * w) behind it."""
    import torch

    def fail(key, **names):
        raise MafError(text[key] % dict(names, what=what))

    if torch.is_tensor(frames):
        if frames.dim() != 4:
            fail("batch", shape=tuple(frames.shape))
        frames = list(frames.unbind(0))
    frames = list(frames)
    if not frames:
        fail("none")
    for i, f in enumerate(frames):
        if not torch.is_tensor(f):
            fail("not_tensor", i=i, kind=type(f).__name__)
        if not f.is_cuda:
            fail("cpu", i=i, device=f.device)
        if "device" in text and f.device != frames[0].device:
            fail("device", i=i, device=f.device, first=frames[0].device)
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
            fail("type", i=i, dtype=f.dtype, shape=tuple(f.shape))
        h, w = int(f.shape[0]), int(f.shape[1])
        if "empty" in text and (h == 0 or w == 0):
            fail("empty", i=i, w=w, h=h)
        if "too_large" in text and (h > 65535 or w > 65535):
            fail("too_large", i=i, w=w, h=h)
        if f.stride(2) != 1 or f.stride(1) != 3:
            fail("stride", i=i, strides=tuple(f.stride()))
        if "pitch" in text and h > 1 and f.stride(0) < 3 * w:
            fail("pitch", i=i, strides=tuple(f.stride()))
    return frames


def rect_list(frames, rects, what, kind):
    """The rectangles an encoder (`what`: its name in messages; `kind`: "JPEG" or "PNG") writes one file each for -> int64 arrays (frame index, x1,
    y1, x2, y2).  rects None: every frame whole; else a host int array (or tensor) [R, 5] of (frame index, x1, y1, x2, y2), each inside its frame
    and not empty."""
    import torch
    fh = np.array([f.shape[0] for f in frames], np.int64)
    fw = np.array([f.shape[1] for f in frames], np.int64)
    if rects is None:
        return np.arange(len(frames)), np.zeros_like(fw), np.zeros_like(fh), fw, fh
    ra = np.asarray(rects.cpu() if isinstance(rects, torch.Tensor) else rects)
    if ra.ndim != 2 or ra.shape[1] != 5 or ra.dtype.kind not in "iu":
        raise MafError("%s: rects is an integer array [R, 5] of (frame index, x1, y1, x2, y2)" % what)
    if ra.shape[0] == 0:
        raise MafError("%s: no rectangles" % what)
    fi, x1, y1, x2, y2 = (ra[:, c].astype(np.int64) for c in range(5))
    bad = np.flatnonzero((fi < 0) | (fi >= len(frames)))
    if bad.size:
        raise MafError("%s: rectangle %d names frame %d of %d" % (what, bad[0], fi[bad[0]], len(frames)))
    bad = np.flatnonzero((x1 < 0) | (y1 < 0) | (x2 > fw[fi]) | (y2 > fh[fi]))
    if bad.size:
        k = int(bad[0])
        raise MafError("%s: rectangle %d (%d, %d, %d, %d) lies outside its %d x %d frame" % (what, k, x1[k], y1[k], x2[k], y2[k], fw[fi[k]], fh[fi[k]]))
    bad = np.flatnonzero((x2 <= x1) | (y2 <= y1))
    if bad.size:
        k = int(bad[0])
        raise MafError("%s: rectangle %d (%d, %d, %d, %d) is empty: there is no %s file of an empty image" % (what, k, x1[k], y1[k], x2[k], y2[k], kind))
    return fi, x1, y1, x2, y2
