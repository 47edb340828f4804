"""Frames in, detections in source-frame pixels out, on the device ("optional GPU letterbox").

The layer in front of Model.forward and behind non_max_suppression that the reference runs on the host with OpenCV, one image at a time:
  * letterbox(frames, ...)   letterbox() (yolov6/data/data_augment.py:53-82) + the HWC -> CHW / BGR -> RGB of Inferer.precess_image
                             (yolov6/core/inferer.py:169-179) for a batch: ONE kernel (csrc/letterbox.hip) writing the uint8 NCHW batch the
                             engine takes (the / 255 stays folded into the stem);
  * eval_batch(frames, ...)  TrainValDataset.load_image + the rect letterbox of __getitem__ (yolov6/data/datasets.py:277-300, :196-213) with
                             the batch shape of sort_files_shapes (:670-695): (imgs, shapes) as collate_fn hands them to the Evaler;
  * resize_area(frames, sizes)  load_image's cv2.resize INTER_AREA of evaluation frames larger than the load size (datasets.py:294-300, r < 1):
                             ONE kernel (csrc/resize_area.hip) for a list of frames; eval_batch(area=True) runs it in front of the letterbox
                             launch for the frames that need it (opt-in: without the flag such frames raise MafError as before);
  * rescale_boxes(dets, ...) Inferer.rescale (inferer.py:181-195) + .round() (:98), in place on the device;
  * detect_frames(model, frames, ...)  the Inferer.infer loop (inferer.py:71-98) for a batch: letterbox -> model -> NMS -> rescale, one
                             device -> host copy (the per-image counts).
The geometry (scale, unpadded size, padding) is host bookkeeping with the reference's own formulas, Python's round-half-even round() included
(tests/golden/letterbox_cases.npz holds what the reference's code computes).  The pixels follow OpenCV's uint8 INTER_LINEAR as restated in
tests/letterbox_ref.py and its uint8 INTER_AREA as restated in tests/area_ref.py, bit for bit.  No CPU fallback: CPU or non-uint8 frames raise MafError.
"""
import math
from functools import partial

import numpy as np
import torch

from . import lib, staging
from .lib import MafError
from .nms import NmsHandle, nms_raw


# ---------------------------------------------------------------- geometry (host)

def check_img_size(img_size, s=32, floor=0):
    """Inferer.check_img_size (inferer.py:197-215) without the warning: an int or [h, w] list rounded UP to multiples of s -> [h, w]."""
    if isinstance(img_size, int):
        n = max(math.ceil(img_size / int(s)) * int(s), floor)
        return [n, n]
    if isinstance(img_size, (list, tuple)):
        return [max(math.ceil(x / int(s)) * int(s), floor) for x in img_size]
    raise Exception(f"Unsupported type of img_size: {type(img_size)}")


def letterbox_geometry(h, w, new_shape=(640, 640), auto=True, scaleup=True, stride=32, return_int=False):
    """letterbox() of data_augment.py:53-82 for a frame of h x w, without the pixels.
    -> dict(r, new_unpad=(w', h'), top, bottom, left, right, shape=(H, W), ret=(r, (dw, dh)) or (r, (left, top)) with return_int)."""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / h, new_shape[1] / w)
    if not scaleup:
        r = min(r, 1.0)
    new_unpad = int(round(w * r)), int(round(h * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:
        dw, dh = dw % stride, dh % stride                   # np.mod of two ints: same value, same sign rule as Python's %
    dw /= 2
    dh /= 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return dict(r=r, new_unpad=new_unpad, top=top, bottom=bottom, left=left, right=right,
                shape=(new_unpad[1] + top + bottom, new_unpad[0] + left + right),
                ret=(r, (left, top)) if return_int else (r, (dw, dh)))


def load_image_size(h0, w0, img_size=640, load_size=None, area=False):
    """TrainValDataset.load_image (datasets.py:277-300) in evaluation (augment = False), without the pixels -> (r, (h, w)).  `load_size` is
    the reference's force_load_size (hyp["test_load_size"]; None: img_size).  r < 1 means OpenCV INTER_AREA in the reference: MafError unless
    area=True (resize_area does it then)."""
    r = (load_size if load_size else img_size) / max(h0, w0)
    if r < 1:
        if not area:
            raise MafError("eval_batch: a %d x %d frame is larger than img_size = %d: the reference shrinks it with OpenCV INTER_AREA, which this "
                           "package does not implement (frames up to img_size on the longest side: COCO val is covered)"
                           % (h0, w0, load_size if load_size else img_size))
        h, w = int(h0 * r), int(w0 * r)
        if h < 1 or w < 1:
            raise MafError("eval_batch: a %d x %d frame shrinks to %d x %d at load size %d: cv2.resize fails on an empty size"
                           % (h0, w0, h, w, load_size if load_size else img_size))
        return r, (h, w)
    if r != 1:
        return r, (int(h0 * r), int(w0 * r))
    return r, (h0, w0)


def rect_batch_shape(hw0, img_size=640, stride=32, pad=0.5):
    """TrainValDataset.sort_files_shapes (datasets.py:670-695) for ONE batch holding frames of the original sizes hw0 = [(h0, w0), ...]:
    ceil(shape * img_size / stride + pad) * stride -> [H, W] (pad 0.5 for val, evaler.py:122-129)."""
    ar = np.array([h / w for h, w in hw0])
    mini, maxi = ar.min(), ar.max()
    shape = [1, 1]
    if maxi < 1:
        shape = [maxi, 1]
    elif mini > 1:
        shape = [1, 1 / mini]
    return (np.ceil(np.array(shape) * img_size / stride + pad).astype(np.int64) * stride).tolist()


def eval_geometry(h0, w0, batch_shape, img_size=640, load_size=None, return_int=False, area=False):
    """load_image + letterbox(img, batch_shape, auto=False, scaleup=False) of __getitem__ -> dict(new_unpad, top, left, shape, shapes, load):
    `shapes` = ((h0, w0), ((h * ratio / h0, w * ratio / w0), pad)), what convert_to_coco_format consumes; `return_int` makes pad the
    (left, top) of hyp["letterbox_return_int"]; `load` names load_image's resize: "area" (r < 1, needs area=True), "linear" (r > 1) or None.
    A frame that took the area path may be shrunk again by the letterbox (two resizes, as the reference does); any other frame may not."""
    r, (h, w) = load_image_size(h0, w0, img_size, load_size, area)
    load = "area" if r < 1 else ("linear" if r != 1 else None)
    g = letterbox_geometry(h, w, tuple(batch_shape), auto=False, scaleup=False, return_int=return_int)
    if g["new_unpad"] != (w, h) and load != "area":
        raise MafError("eval_batch: batch shape %s is smaller than the %d x %d loaded frame: the reference would resize twice (load_image, then "
                       "letterbox); not supported" % (list(batch_shape), h, w))
    ratio, pad = g["ret"]
    g["shapes"] = ((h0, w0), ((h * ratio / h0, w * ratio / w0), pad))
    g["load_hw"] = (h, w)
    g["load"] = load
    return g


# ---------------------------------------------------------------- INTER_AREA tables (host)

DBL_EPSILON = float(np.finfo(np.float64).eps)
# maf_area_frame_t (include/mafyolo_hip.h)
AREA_FRAME_DT = np.dtype([("src", "<u8"), ("src_pitch", "<i8"), ("h", "<i4"), ("w", "<i4"), ("dst", "<u8"), ("new_h", "<i4"), ("new_w", "<i4"),
                          ("path", "<i4"), ("iscale_x", "<i4"), ("iscale_y", "<i4"), ("inv_area", "<f4"),
                          ("x_start", "<i4"), ("x_pairs", "<i4"), ("y_start", "<i4"), ("y_pairs", "<i4")], align=True)


def area_plan(h, w, new_h, new_w):
    """The path cv2.resize(..., INTER_AREA) takes for h x w -> new_h x new_w (both axes shrink or stay), by OpenCV's own test in double:
    scale = 1.0 / (new / old), iscale = round-half-even(scale), fast when |scale - iscale| < DBL_EPSILON on both axes
    -> (lib.AREA_FAST2 | AREA_FASTN | AREA_GENERAL, iscale_x, iscale_y)."""
    scale_x, scale_y = 1.0 / (new_w / w), 1.0 / (new_h / h)
    ix, iy = int(round(scale_x)), int(round(scale_y))
    if abs(scale_x - ix) < DBL_EPSILON and abs(scale_y - iy) < DBL_EPSILON:
        if ix * new_w != w or iy * new_h != h:
            raise MafError("resize_area: %d x %d -> %d x %d passes OpenCV's integer-factor test without exact factors" % (h, w, new_h, new_w))
        return (lib.AREA_FAST2 if ix == 2 and iy == 2 else lib.AREA_FASTN), ix, iy
    return lib.AREA_GENERAL, ix, iy


def area_table(n_src, n_dst):
    """OpenCV's computeResizeAreaTab for one axis, in double -> (start int32 [n_dst + 1], src index int32 [k], alpha float32 [k]): destination
    index d owns entries start[d] .. start[d + 1] - 1, in OpenCV's order (the partial source cell in front, the whole cells, the partial
    cell behind; a partial cell counts when it is wider than 1e-3)."""
    scale = 1.0 / (n_dst / n_src)
    d = np.arange(n_dst, dtype=np.float64)
    f1 = d * scale
    f2 = f1 + scale
    cell = np.minimum(scale, n_src - f1)
    s2 = np.minimum(np.floor(f2).astype(np.int64), n_src - 1)
    s1 = np.minimum(np.ceil(f1).astype(np.int64), s2)
    head, tail, mid = (s1 - f1) > 1e-3, (f2 - s2) > 1e-3, s2 - s1
    count = head + mid + tail
    if (count < 1).any() or (mid < 0).any():
        raise MafError("resize_area: %d -> %d leaves a destination index without a source cell" % (n_src, n_dst))
    start = np.concatenate([[0], np.cumsum(count)])
    si, alpha = np.empty(start[-1], np.int64), np.empty(start[-1], np.float64)
    pos = start[:-1]
    si[pos[head]], alpha[pos[head]] = s1[head] - 1, ((s1 - f1) / cell)[head]
    rep = np.repeat(np.arange(n_dst), mid)
    j = np.arange(rep.size) - np.repeat(np.cumsum(mid) - mid, mid)
    at = pos[rep] + head[rep] + j
    si[at], alpha[at] = s1[rep] + j, (1.0 / cell)[rep]
    at = (pos + head + mid)[tail]
    si[at], alpha[at] = s2[tail], (np.minimum(np.minimum(f2 - s2, 1.0), cell) / cell)[tail]
    if si.min() < 0 or si.max() >= n_src:
        raise MafError("resize_area: %d -> %d names a source index outside the frame" % (n_src, n_dst))
    return start.astype(np.int32), si.astype(np.int32), alpha.astype(np.float32)


# ---------------------------------------------------------------- device

_FRAME_TEXT = {      # staging.frame_list in this module's words; `what` names the entry point
    "batch": "letterbox: a single tensor of frames is uint8 [B, h, w, 3]",
    "none": "letterbox: no frames",
    "not_tensor": "%(what)s runs on the HIP path only: frames must be CUDA tensors (no CPU fallback)",
    "cpu": "%(what)s runs on the HIP path only: frames must be CUDA tensors (no CPU fallback)",
    "type": "letterbox: frames are uint8 [h, w, 3] tensors, got %(dtype)s %(shape)s",
    "stride": "letterbox: a frame needs pixel stride 3 and channel stride 1 (rows may have any pitch)"}


def _frame_list(frames, what="letterbox"):
    return staging.frame_list(frames, _FRAME_TEXT, what)


def _launch(frames, H, W, geoms, color, bgr):
    from . import torch_ops
    geometry = []
    for g in geoms:
        geometry += [g["new_unpad"][1], g["new_unpad"][0], g["top"], g["left"]]
    return torch_ops.load().letterbox(frames, int(H), int(W), geometry, [int(c) for c in color], bool(bgr))


def _check_one_shape(geoms):
    shapes = {g["shape"] for g in geoms}
    if len(shapes) > 1:
        raise ValueError("letterbox: with auto=True the frames of this batch letterbox to different shapes %s; a batch shares one shape — "
                         "pass auto=False (pad to the full new_shape) or batch frames of one aspect ratio" % sorted(shapes))
    return shapes.pop()


def letterbox(frames, new_shape=640, color=(114, 114, 114), auto=True, scaleup=True, stride=32, bgr=True):
    """The reference's letterbox + precess_image for a batch.  frames: a list of uint8 [h_i, w_i, 3] CUDA tensors (views and crops welcome)
    or one uint8 [B, h, w, 3] tensor; `color` in the frames' channel order.  -> (imgs uint8 [B, 3, H, W] RGB, ratios [B], pads [B] of (dw, dh)):
    the reference's return triple per frame.  `new_shape` goes through Inferer.check_img_size first.  All frames of a batch share one H x W:
    with auto=True frames of different aspect can letterbox to different shapes, which raises ValueError (pass auto=False to pad every frame
    to the full new_shape)."""
    frames = _frame_list(frames)
    ns = check_img_size(new_shape if isinstance(new_shape, int) else list(new_shape), stride)
    by_size = {}                                          # frames of one size share their geometry (a video batch: one entry)
    geoms = []
    for f in frames:
        hw = (int(f.shape[0]), int(f.shape[1]))
        if hw not in by_size:
            by_size[hw] = letterbox_geometry(hw[0], hw[1], tuple(ns), auto, scaleup, stride)
        geoms.append(by_size[hw])
    H, W = _check_one_shape(geoms)
    imgs = _launch(frames, H, W, geoms, color, bgr)
    return imgs, [g["ret"][0] for g in geoms], [g["ret"][1] for g in geoms]


def _area_tables(frames, sizes):
    """The host half of resize_area -> (frame table [n] of AREA_FRAME_DT with dst as an offset into the output, the table words int32 [k],
    output bytes): paths by area_plan, one decimation-table set per distinct (source, destination) size pair of an axis."""
    tab = np.zeros(len(frames), AREA_FRAME_DT)
    words, at, n_words, off = [], {}, 0, 0

    def axis(n_src, n_dst):
        nonlocal n_words
        if (n_src, n_dst) not in at:
            start, si, alpha = area_table(n_src, n_dst)
            pairs = np.empty(2 * si.size, np.int32)
            pairs[0::2], pairs[1::2] = si, alpha.view(np.int32)
            pad = np.zeros((start.size + n_words) & 1, np.int32)           # the pairs start on an even word (64-bit loads)
            at[(n_src, n_dst)] = (n_words, n_words + start.size + pad.size)
            words.extend([start, pad, pairs])
            n_words += start.size + pad.size + pairs.size
        return at[(n_src, n_dst)]

    for i, (f, (nh, nw)) in enumerate(zip(frames, sizes)):
        h, w = int(f.shape[0]), int(f.shape[1])
        if nh < 1 or nw < 1 or h < 1 or w < 1:
            raise MafError("resize_area: frame %d: %d x %d -> %d x %d: sizes must be positive" % (i, h, w, nh, nw))
        if nh > h or nw > w:
            raise MafError("resize_area: frame %d: %d x %d -> %d x %d grows an axis (INTER_AREA shrinks; OpenCV turns a growing axis into a "
                           "linear variant, which load_image cannot reach)" % (i, h, w, nh, nw))
        path, ix, iy = area_plan(h, w, nh, nw)
        e = tab[i]
        e["src"], e["src_pitch"], e["h"], e["w"], e["new_h"], e["new_w"] = f.data_ptr(), f.stride(0), h, w, nh, nw
        e["path"], e["iscale_x"], e["iscale_y"] = path, ix, iy
        e["inv_area"] = np.float32(1.0) / np.float32(ix * iy)
        if path == lib.AREA_GENERAL:
            (e["x_start"], e["x_pairs"]), (e["y_start"], e["y_pairs"]) = axis(w, nw), axis(h, nh)
        e["dst"] = off                                                     # + the allocation's address, once it exists
        off += 3 * nh * nw
    return tab, (np.concatenate(words) if words else np.zeros(0, np.int32)), off


_area_library = partial(staging.checked_library, "area", (("maf_area_struct_sizes", 1),), AREA_FRAME_DT.itemsize, "a maf_area_frame_t")


def resize_area(frames, sizes, stream=None):
    """cv2.resize(frame, (new_w, new_h), interpolation=cv2.INTER_AREA) for a list of frames whose axes shrink or stay, in one launch.
    frames: uint8 [h_i, w_i, 3] CUDA tensors (views and crops welcome); sizes: one (new_h, new_w) per frame.  -> a list of uint8
    [new_h_i, new_w_i, 3] tensors, views of one allocation.  The frame table and the decimation tables (one set per distinct size pair)
    travel in one pinned blob with one host -> device copy; nothing synchronises the host.  `stream`: a torch.cuda.Stream to work on
    (default: the current one)."""
    frames = _frame_list(frames, "resize_area")
    sizes = [(int(s[0]), int(s[1])) for s in sizes]
    if len(sizes) != len(frames):
        raise MafError("resize_area: %d sizes for %d frames" % (len(sizes), len(frames)))
    dev = frames[0].device
    if any(f.device != dev for f in frames):
        raise MafError("resize_area: the frames of a call live on one device")
    tab, words, total = _area_tables(frames, sizes)
    L = _area_library()
    tab_bytes = tab.nbytes                                                # a multiple of 8: the table words behind it stay aligned
    with staging.staged(tab_bytes + words.nbytes, dev, stream) as s:
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        tab["dst"] += np.uint64(out.data_ptr())
        s.host[:tab_bytes] = tab.view(np.uint8)
        s.host[tab_bytes:] = words.view(np.uint8)
        blob = s.copy()
        lib.check(L.maf_resize_area(s.host.ctypes.data, blob.data_ptr(), len(frames), s.host.ctypes.data + tab_bytes if words.size else None,
                                    blob.data_ptr() + tab_bytes if words.size else None, words.size, s.stream.cuda_stream))
    res, off = [], 0
    for nh, nw in sizes:
        res.append(out[off:off + 3 * nh * nw].view(nh, nw, 3))
        off += 3 * nh * nw
    return res


def eval_batch(frames, img_size=640, stride=32, pad=0.5, shape=None, bgr=True, area=False, load_size=None, return_int=False, rect=True):
    """The evaluation loader's batch (load_image + rect letterbox + collate_fn) from decoded frames -> (imgs uint8 [B, 3, H, W], shapes): the
    batch shape is `shape` ([H, W]), [img_size, img_size] with rect=False (the reference's not_infer_on_rect), or the sort_files_shapes rule
    over this batch's aspect ratios with `pad` (0.0: force_no_pad); `shapes` is the per-image tuple that EvalLoop / convert_to_coco_format
    consume.  `load_size` is hyp["test_load_size"], `return_int` hyp["letterbox_return_int"].  With area=True the frames whose longest side
    exceeds the load size are shrunk by one resize_area launch (OpenCV INTER_AREA) in front of the letterbox launch, which then copies them,
    or shrinks them again linearly where the batch shape demands it; every other frame takes the single launch as before.  Without
    area=True such frames raise MafError.  The reference's eval_640_repro recipe:
    eval_batch(frames, 640, pad=0.0, rect=False, area=True, load_size=638, return_int=True), then EvalLoop(..., scale_exact=True)."""
    frames = _frame_list(frames, "eval_batch" if area else "letterbox")
    hw0 = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
    if shape is not None:
        bs = list(shape)
    elif not rect:
        bs = [int(img_size), int(img_size)]
    else:
        bs = rect_batch_shape(hw0, img_size, stride, pad)
    geoms = [eval_geometry(h0, w0, bs, img_size, load_size, return_int, area) for h0, w0 in hw0]
    H, W = geoms[0]["shape"]
    shrink = [i for i, g in enumerate(geoms) if g["load"] == "area"]
    if shrink:
        for i, small in zip(shrink, resize_area([frames[i] for i in shrink], [geoms[i]["load_hw"] for i in shrink])):
            frames[i] = small
    imgs = _launch(frames, H, W, geoms, (114, 114, 114), bgr)
    return imgs, tuple(g["shapes"] for g in geoms)


def rescale_params(letterboxed_hw, src_shapes):
    """Inferer.rescale's ratio and padding per frame, in the reference's double arithmetic -> fp32 [B, 5] (h0, w0, ratio, pad_x, pad_y)."""
    H, W = int(letterboxed_hw[0]), int(letterboxed_hw[1])
    par = np.empty((len(src_shapes), 5), np.float32)
    for i, s in enumerate(src_shapes):
        h0, w0 = int(s[0]), int(s[1])
        ratio = min(H / h0, W / w0)
        par[i] = (h0, w0, ratio, (W - w0 * ratio) / 2, (H - h0 * ratio) / 2)
    return par


def rescale_boxes(dets, letterboxed_hw, src_shapes, round=True):
    """Inferer.rescale(img.shape[2:], det[:, :4], img_src.shape).round() for a batch, in place on the device.  `dets` is any result form that
    convert_to_coco_format accepts: the list of [n_i, 6] tensors, the (rows, idx, count) triple of nms_raw, or an NmsHandle.  Returns `dets`."""
    if isinstance(dets, NmsHandle):
        rows, cnt = dets.rows, dets.cnt
        torch.cuda.current_stream(rows.device).wait_event(dets.event)
    elif isinstance(dets, tuple) and len(dets) == 3 and torch.is_tensor(dets[2]):
        rows, _, cnt = dets
    else:
        rows = cnt = None
    if rows is not None:
        if not rows.is_cuda:
            raise MafError("rescale_boxes runs on the HIP path only: got a %s tensor (no CPU fallback)" % rows.device)
        if not rows.is_contiguous():
            raise MafError("rescale_boxes: the rows of an NMS result are contiguous [B, max_det, 6]")
        _rescale(rows, cnt, letterboxed_hw, src_shapes, round)
        return dets
    B = len(dets)
    if B == 0:
        return dets
    dev = dets[0].device
    if not dets[0].is_cuda:
        raise MafError("rescale_boxes runs on the HIP path only: got a %s tensor (no CPU fallback)" % dev)
    md = max(1, max(int(o.shape[0]) for o in dets))
    rows = torch.zeros(B, md, 6, dtype=torch.float32, device=dev)
    for b, o in enumerate(dets):
        rows[b, :o.shape[0]] = o
    cnt = staging.upload(np.array([int(o.shape[0]) for o in dets], np.int32), dev)
    _rescale(rows, cnt, letterboxed_hw, src_shapes, round)
    for b, o in enumerate(dets):
        o[:, :4] = rows[b, :o.shape[0], :4]
    return dets


def _rescale(rows, cnt, letterboxed_hw, src_shapes, do_round):
    B, max_det, stride = rows.shape
    if len(src_shapes) != B:
        raise MafError("rescale_boxes: %d source shapes for %d images" % (len(src_shapes), B))
    par = staging.upload(rescale_params(letterboxed_hw, src_shapes), rows.device)
    st = torch.cuda.current_stream(rows.device)
    lib.check(lib.load().maf_rescale_boxes(rows.data_ptr(), cnt.data_ptr(), B, max_det, stride, par.data_ptr(), int(bool(do_round)), st.cuda_stream))


def detect_frames(model, frames, img_size=640, conf_thres=0.4, iou_thres=0.45, classes=None, agnostic=False, max_det=1000,
                  auto=True, stride=32, bgr=True):
    """Inferer.infer (inferer.py:71-98) for a batch of frames: letterbox -> model(imgs) -> non_max_suppression -> rescale(...).round().
    -> the reference's list of [n_i, 6] tensors (x1, y1, x2, y2, conf, cls) in source-frame pixels, on the device; the one host sync is the
    copy of the per-image counts.  auto=True letterboxes like the Inferer (minimum rectangle: frames of one aspect ratio per batch);
    auto=False pads every frame to the full img_size square.  The forward's precision is the model's (Model.precision); the uint8 batch goes in
    as it is (the / 255 is folded into the stem)."""
    imgs, _, _ = letterbox(frames, img_size, auto=auto, stride=stride, bgr=bgr)
    frames = _frame_list(frames)
    with torch.no_grad():
        pred = model(imgs)[0]
    rows, idx, cnt = nms_raw(pred, conf_thres, iou_thres, classes, agnostic, max_det=max_det)
    _rescale(rows, cnt, imgs.shape[2:], [(int(f.shape[0]), int(f.shape[1])) for f in frames], True)
    counts = cnt.tolist()                                  # the one device -> host copy
    return [rows[b, :n] for b, n in enumerate(counts)]
