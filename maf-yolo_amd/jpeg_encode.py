"""Frames in, file bytes out, on the device: baseline JPEG encoding that equals libjpeg with its defaults bit for bit.

The last step of the reference's tools/infer.py, which it runs on the host one picture at a time: save_one_box(..., BGR=True) for every
detection and cv2.imwrite(save_path, img_src) for the frame (yolov6/core/inferer.py):
  * crop_rects(det, shape)  host only: the rectangle save_one_box cuts out for each box (same float32 operations in the same order);
  * encode(frames, ...)     a list of uint8 [h, w, 3] BGR CUDA tensors (or one [B, h, w, 3]), optionally rectangles of them -> EncodedBatch:
                            ONE pinned staging buffer, ONE host -> device copy, one chain of launches for the whole call
                            (csrc/jpeg_encode.hip), no host synchronisation;
  * EncodedBatch.files()    -> list[bytes]; the only call that synchronises: one read of the lengths, one of the used part of the buffer.
What is written: baseline sequential DCT (SOF0), 8 bit, three components, 4:2:0 (libjpeg's default) or 4:4:4, jpeg_set_quality tables with
force_baseline, JDCT_ISLOW, the standard Huffman tables (no optimisation), JFIF 1.01 header (units 0, density 1 x 1), no restart markers.
The rules are restated in tests/jpeg_encode_ref.py and pinned there to files Pillow (libjpeg-turbo) wrote.  These are also the settings
OpenCV documents for cv2.imwrite (quality 95, 2 x 2 chroma sampling), but byte identity with cv2.imwrite itself has not been checked by
anyone: parity is claimed with libjpeg as Pillow drives it only.  No CPU fallback.
Not done: grayscale output, 4:2:2, optimised Huffman tables, progressive output, restart intervals, EXIF, drawing boxes or text on frames
(plot_box_and_label), video.
"""
from functools import partial

import numpy as np

from . import lib, staging
from .lib import MafError

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63],
                  np.int64)

# ITU-T T.81 Annex K.1 (jcparam.c std_luminance_quant_tbl / std_chrominance_quant_tbl), natural order
QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                      np.int64)
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                        + [99] * 32, np.int64)


def _ac_values(head, first_rows):
    """The value list of an Annex K.3 AC table: its irregular head, then run/size bytes row by row (`first_rows`: the first size of the
    rows 1.. of the tail; every row runs to size 10)."""
    return head + [16 * r + s for r, s0 in first_rows for s in range(s0, 11)]


# ITU-T T.81 Annex K.3 (jcparam.c std_huff_tables): (codes per length 1..16, values in code order); DC luma, DC chroma, AC luma, AC chroma
HUFFMAN = (
    ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
     _ac_values([0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
                 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A],
                [(1, 6), (2, 5), (3, 4), (4, 3), (5, 3), (6, 3), (7, 3), (8, 3), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 1), (15, 1)])),
    ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
     _ac_values([0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
                 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18,
                 0x19, 0x1A],
                [(2, 6), (3, 5), (4, 3), (5, 3), (6, 3), (7, 3), (8, 2), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 2), (15, 2)])),
)

BLOCK_BITS = 1660             # MAF_JPEG_ENC_BLOCK_BITS: see _worst_case_bytes
BLOCK_BYTES = 208             # MAF_JPEG_ENC_BLOCK_BYTES
CHUNK = 4096                  # MAF_JPEG_ENC_CHUNK
MAX_BLOCKS = 1 << 20          # MAF_JPEG_ENC_MAX_BLOCKS
SAMPLING = {"4:2:0": 2, "4:4:4": 1}

HEADER_DT = np.dtype([("n_files", "<i4"), ("n_blocks", "<i4"), ("n_chunks", "<i4"), ("reserved", "<i4"), ("jobs_off", "<i8"), ("huff_off", "<i8"),
                      ("quant_off", "<i8"), ("heads_off", "<i8"), ("heads_bytes", "<i8"), ("total_bytes", "<i8"), ("out_bytes", "<i8")])   # maf_jpeg_enc_header_t
JOB_DT = np.dtype([("src", "<u8"), ("pitch", "<i8"), ("w", "<i4"), ("h", "<i4"), ("hs", "<i4"), ("mcux", "<i4"), ("mcuy", "<i4"), ("block0", "<i4"),
                   ("n_blocks", "<i4"), ("chunk0", "<i4"), ("n_chunks", "<i4"), ("head_off", "<i4"), ("head_len", "<i4"), ("reserved", "<i4")])   # maf_jpeg_enc_job_t


def quant_table(base, quality):
    """jcparam.c jpeg_set_quality -> jpeg_add_quant_table with force_baseline: the table of `quality` (1..100), natural order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255)


def huff_code_table(bits, vals):
    """jchuff.c jpeg_make_c_derived_tbl in the layout the kernels read: uint32 [256], length << 16 | code per symbol, 0 where it has none."""
    out = np.zeros(256, np.uint32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (length << 16) | code
            code += 1
            k += 1
        code <<= 1
    return out


def file_header(w, h, hs, qluma, qchroma):
    """jcmarker.c write_file_header + write_frame_header + write_scan_header: SOI, APP0 (JFIF 1.01, units 0, density 1 x 1), DQT 0, DQT 1, SOF0,
    DHT DC 0, AC 0, DC 1, AC 1, SOS."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)
    out = [b"\xff\xd8", seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    out += [seg(0xDB, bytes([i]) + bytes(q[ZIGZAG].astype(np.uint8))) for i, q in enumerate((qluma, qchroma))]
    out.append(seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 16 * hs + hs, 0, 2, 0x11, 1, 3, 0x11, 1])))
    out += [seg(0xC4, bytes([sel]) + bytes(HUFFMAN[t][0]) + bytes(HUFFMAN[t][1])) for sel, t in ((0x00, 0), (0x10, 2), (0x01, 1), (0x11, 3))]
    out.append(seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


def crop_rects(det, shape, gain=1.02, pad=10, square=False):
    """The rectangles save_one_box (yolov6/core/inferer.py) cuts out of a frame of `shape` (h, w, ...) for the xyxy boxes det [R, 4+] (host
    tensor or array): xyxy2xywh, wh * gain + pad, xywh2xyxy, .long() (truncation toward zero), clip to the frame, in torch float32 as there.
    -> int64 [R, 4] (x1, y1, x2, y2) on the host; frame[y1:y2, x1:x2] is the crop (it can be empty: encode() refuses such a rectangle)."""
    import torch
    d = det.detach().cpu().to(torch.float32) if isinstance(det, torch.Tensor) else torch.from_numpy(np.array(det, dtype=np.float32))
    if d.dim() == 0 or d.shape[-1] < 4:
        raise MafError("jpeg_encode.crop_rects: det is [R, 4+] xyxy boxes, got shape %s" % (tuple(d.shape),))
    x = d.reshape(-1, d.shape[-1])[:, :4]
    b = x.clone()
    b[:, 0] = (x[:, 0] + x[:, 2]) / 2
    b[:, 1] = (x[:, 1] + x[:, 3]) / 2
    b[:, 2] = x[:, 2] - x[:, 0]
    b[:, 3] = x[:, 3] - x[:, 1]
    if square:
        b[:, 2:] = b[:, 2:].max(1)[0].unsqueeze(1)
    b[:, 2:] = b[:, 2:] * gain + pad
    y = b.clone()
    y[:, 0] = b[:, 0] - b[:, 2] / 2
    y[:, 1] = b[:, 1] - b[:, 3] / 2
    y[:, 2] = b[:, 0] + b[:, 2] / 2
    y[:, 3] = b[:, 1] + b[:, 3] / 2
    r = y.long()
    r[:, 0].clamp_(0, shape[1])
    r[:, 1].clamp_(0, shape[0])
    r[:, 2].clamp_(0, shape[1])
    r[:, 3].clamp_(0, shape[0])
    return r.numpy()


def _worst_case_bytes(n_blocks):
    """Bytes the entropy-coded segment of `n_blocks` blocks can take before stuffing.  No block costs more than BLOCK_BITS = 22 + 63 * 26:
    the longest DC code (11 bits, category 11 of the chroma table) with its 11 value bits, and for each of the 63 AC coefficients the
    longest code of the standard tables (16 bits) with 10 value bits — the code lengths a block of quality 100 can reach; a ZRL (11 bits)
    stands for 16 coefficients and is cheaper than they would be.  That is 208 bytes per block; stuffing (0x00 behind every 0xFF) at most
    doubles it, which is what the output buffer is sized by."""
    return BLOCK_BYTES * n_blocks


class EncodedBatch:
    """The files of one encode() call on the device: `buffer` (uint8; the files back to back from byte 0), `offsets` (int64 [n]) and
    `lengths` (int32 [n]).  Nothing has synchronised yet; files() does."""

    def __init__(self, buffer, offsets, lengths, stream, keep):
        self.buffer, self.offsets, self.lengths, self.stream = buffer, offsets, lengths, stream
        self._keep = keep             # the frames, the staging buffer and the scratch: alive until the work that reads them is done
        self._files = None

    def __len__(self):
        return int(self.lengths.shape[0])

    def files(self):
        """-> list[bytes], one JPEG file per frame or rectangle.  One read of the lengths, one read of the used part of the buffer."""
        if self._files is None:
            import torch
            with torch.cuda.stream(self.stream):
                lengths = self.lengths.cpu().numpy().astype(np.int64)        # synchronises: everything the call launched is done
                data = self.buffer[:int(lengths.sum())].cpu().numpy()
            ends = np.cumsum(lengths)
            self._files = [data[e - n:e].tobytes() for e, n in zip(ends.tolist(), lengths.tolist())]
            self._keep = None
        return self._files


_library = partial(staging.checked_library, "jpeg_encode", (("maf_jpeg_encode_struct_sizes", 2),), [HEADER_DT.itemsize, JOB_DT.itemsize],
                   "maf_jpeg_enc_* structs")

_FRAME_TEXT = {      # staging.frame_list in encode()'s words
    "batch": "jpeg_encode.encode: a tensor of frames is [B, h, w, 3], got %(shape)s",
    "none": "jpeg_encode.encode: no frames",
    "not_tensor": "jpeg_encode.encode: frame %(i)d is a %(kind)s, not a CUDA tensor",
    "cpu": "jpeg_encode.encode runs on the HIP path only (no CPU fallback): frame %(i)d is on %(device)s",
    "device": "jpeg_encode.encode: frame %(i)d is on %(device)s, frame 0 on %(first)s",
    "type": "jpeg_encode.encode: frame %(i)d must be uint8 [h, w, 3] BGR, got %(dtype)s %(shape)s",
    "empty": "jpeg_encode.encode: frame %(i)d is empty (%(w)d x %(h)d): there is no JPEG file of an empty image",
    "too_large": "jpeg_encode.encode: frame %(i)d is %(w)d x %(h)d, a JPEG dimension is at most 65535",
    "stride": "jpeg_encode.encode: frame %(i)d must have pixel stride 3 and channel stride 1 (any row pitch of at least 3 * w), got strides %(strides)s"}
_FRAME_TEXT["pitch"] = _FRAME_TEXT["stride"]


def encode(frames, quality=95, subsampling="4:2:0", rects=None, stream=None, taps=None):
    """Encode frames (a list of uint8 [h, w, 3] BGR CUDA tensors of any sizes, or one [B, h, w, 3] tensor; pixel stride 3, channel stride 1, any row
    pitch: read in place) to baseline JPEG files on the device -> EncodedBatch.  `rects`: a host int array [R, 5] of (frame index, x1, y1, x2,
    y2): one file per rectangle frame[y1:y2, x1:x2] (crop_rects gives save_one_box's) instead of one per frame.  `quality` 1..100 (cv2.imwrite's
    default is 95), `subsampling` "4:2:0" (libjpeg's and cv2's default) or "4:4:4".  `stream`: a torch.cuda.Stream to work on (default: the
    current one).  Every size is known on the host, so nothing is read back here.  `taps`: a dict that receives the intermediate buffers
    (coef, bits, bitoff, packed, the job table, the header) — tests and the probe."""
    import torch
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise MafError("jpeg_encode.encode: quality is an integer from 1 to 100, got %r" % (quality,))
    if subsampling not in SAMPLING:
        raise MafError("jpeg_encode.encode: subsampling is \"4:2:0\" or \"4:4:4\", got %r (4:2:2 and grayscale are not written)" % (subsampling,))
    quality, hs = int(quality), SAMPLING[subsampling]
    frames = staging.frame_list(frames, _FRAME_TEXT)
    fi, x1, y1, x2, y2 = staging.rect_list(frames, rects, "jpeg_encode.encode", "JPEG")
    fw = np.array([f.shape[1] for f in frames], np.int64)
    n = len(fi)
    if n > staging.MAX_FILES:
        raise MafError("jpeg_encode.encode takes up to 65535 files per call")
    qluma, qchroma = quant_table(QUANT_LUMA, quality), quant_table(QUANT_CHROMA, quality)
    w, h = x2 - x1, y2 - y1
    pitch = np.maximum(np.array([f.stride(0) for f in frames], np.int64), 3 * fw)[fi]      # a one-row frame may carry any stride 0: it is never used
    base = np.array([f.data_ptr() for f in frames], np.uint64)[fi]
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * hs))
    nb = mcux * mcuy * (hs * hs + 2)
    if nb.max() > MAX_BLOCKS:
        k = int(nb.argmax())
        raise MafError("jpeg_encode.encode: file %d (%d x %d) has %d blocks, at most %d are taken" % (k, w[k], h[k], nb[k], MAX_BLOCKS))
    nc = -(-_worst_case_bytes(nb) // CHUNK)
    block, chunk = int(nb.sum()), int(nc.sum())
    if block >= 1 << 30 or chunk >= 1 << 30:
        raise MafError("jpeg_encode.encode: %d blocks in one call, fewer than 2^30 are taken (split the batch)" % block)
    head = np.frombuffer(file_header(1, 1, hs, qluma, qchroma), np.uint8)    # the files' headers differ in the four size bytes of SOF0 only
    at = bytes(head).index(b"\xff\xc0") + 5
    heads = np.tile(head, (n, 1))
    heads[:, at], heads[:, at + 1], heads[:, at + 2], heads[:, at + 3] = h >> 8, h & 255, w >> 8, w & 255
    jobs = np.zeros(n, JOB_DT)
    jobs["src"] = base + (y1 * pitch + 3 * x1).astype(np.uint64)
    jobs["pitch"], jobs["w"], jobs["h"], jobs["hs"], jobs["mcux"], jobs["mcuy"] = pitch, w, h, hs, mcux, mcuy
    jobs["block0"], jobs["n_blocks"] = np.cumsum(nb) - nb, nb
    jobs["chunk0"], jobs["n_chunks"] = np.cumsum(nc) - nc, nc
    jobs["head_off"], jobs["head_len"] = np.arange(n) * head.size, head.size
    out_bytes = int((head.size + 2 + 2 * _worst_case_bytes(nb)).sum())      # per file: header + EOI + the stuffed worst case
    codes = np.concatenate([huff_code_table(*t) for t in HUFFMAN])
    quant = np.stack([qluma, qchroma]).astype(np.uint16)
    head_bytes = heads.reshape(-1)
    sections = (("jobs_off", jobs), ("huff_off", codes), ("quant_off", quant), ("heads_off", head_bytes))
    hdr, off = staging.blob_layout(HEADER_DT, sections)
    hdr["n_files"], hdr["n_blocks"], hdr["n_chunks"] = n, block, chunk
    hdr["heads_bytes"], hdr["total_bytes"], hdr["out_bytes"] = head_bytes.nbytes, off, out_bytes
    if off >= staging.MAX_BLOB:
        raise MafError("jpeg_encode.encode: the job table of one call is limited to 2 GiB")
    L = _library()
    dev = frames[0].device
    if stream is not None:
        for f in frames:
            f.record_stream(stream)                                          # the allocator must not hand a dropped frame on while `stream` still reads it
    with staging.staged(off, dev, stream, zeros=True) as s:                  # zeros: the alignment gaps are defined bytes
        staging.write_blob(s.host, hdr, sections)
        blob = s.copy()
        n_sums = -(-block // 256)
        coef = torch.empty(64 * block, dtype=torch.int16, device=dev)
        bits = torch.empty(block, dtype=torch.int32, device=dev)
        bitoff = torch.empty(block + 1, dtype=torch.int64, device=dev)
        sums = torch.empty(2 * n_sums, dtype=torch.int64, device=dev)
        packed = torch.empty(chunk * CHUNK, dtype=torch.uint8, device=dev)   # the worst case of _worst_case_bytes, in whole chunks per file; zeroed by the library on the stream
        ffcount = torch.empty(chunk, dtype=torch.int32, device=dev)
        out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)          # header + EOI + twice the worst case (stuffing) per file; the files are written back to back
        lengths = torch.empty(n, dtype=torch.int32, device=dev)
        offsets = torch.empty(n, dtype=torch.int64, device=dev)
        lib.check(L.maf_jpeg_encode(s.host.ctypes.data, blob.data_ptr(), coef.data_ptr(), bits.data_ptr(), bitoff.data_ptr(), sums.data_ptr(),
                                    packed.data_ptr(), ffcount.data_ptr(), out.data_ptr(), lengths.data_ptr(), offsets.data_ptr(), s.stream.cuda_stream))
    if taps is not None:
        taps.update(coef=coef, bits=bits, bitoff=bitoff, packed=packed, jobs=jobs, header=hdr, quant=quant)
    return EncodedBatch(out, offsets, lengths, s.stream, (frames, s.pinned, blob, coef, bits, bitoff, sums, packed, ffcount))
