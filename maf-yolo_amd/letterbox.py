"""Frames in, detections in source-frame pixels out, on the device ("optional GPU letterbox").

The layer in front of Model.forward and behind non_max_suppression that the reference runs on the host with OpenCV, one image at a time:
  * letterbox(frames, ...)   letterbox() (yolov6/data/data_augment.py:53-82) + the HWC -> CHW / BGR -> RGB of Inferer.precess_image
                             (yolov6/core/inferer.py:169-179) for a batch: ONE kernel (csrc/letterbox.hip) writing the uint8 NCHW batch the
                             engine takes (the / 255 stays folded into the stem);
  * eval_batch(frames, ...)  TrainValDataset.load_image + the rect letterbox of __getitem__ (yolov6/data/datasets.py:277-300, :196-213) with
                             the batch shape of sort_files_shapes (:670-695): (imgs, shapes) as collate_fn hands them to the Evaler;
  * rescale_boxes(dets, ...) Inferer.rescale (inferer.py:181-195) + .round() (:98), in place on the device;
  * detect_frames(model, frames, ...)  the Inferer.infer loop (inferer.py:71-98) for a batch: letterbox -> model -> NMS -> rescale, one
                             device -> host copy (the per-image counts).
The geometry (scale, unpadded size, padding) is host bookkeeping with the reference's own formulas, Python's round-half-even round() included
(tests/golden/letterbox_cases.npz holds what the reference's code computes).  The pixels follow OpenCV's uint8 INTER_LINEAR as restated in
tests/letterbox_ref.py, bit for bit.  No CPU fallback: CPU or non-uint8 frames raise MafError.
"""
import math

import numpy as np
import torch

from . import lib
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


def load_image_size(h0, w0, img_size=640):
    """TrainValDataset.load_image (datasets.py:277-300) in evaluation (augment = False), without the pixels -> (r, (h, w)).  r < 1 means
    OpenCV INTER_AREA with a non-integer factor in the reference: out of scope here (MafError)."""
    r = img_size / max(h0, w0)
    if r < 1:
        raise MafError("eval_batch: a %d x %d frame is larger than img_size = %d: the reference shrinks it with OpenCV INTER_AREA, which this "
                       "package does not implement (frames up to img_size on the longest side: COCO val is covered)" % (h0, w0, img_size))
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


def eval_geometry(h0, w0, batch_shape, img_size=640):
    """load_image + letterbox(img, batch_shape, auto=False, scaleup=False) of __getitem__ -> dict(new_unpad, top, left, shape, shapes):
    `shapes` = ((h0, w0), ((h * ratio / h0, w * ratio / w0), pad)), what convert_to_coco_format consumes."""
    _, (h, w) = load_image_size(h0, w0, img_size)
    g = letterbox_geometry(h, w, tuple(batch_shape), auto=False, scaleup=False)
    if g["new_unpad"] != (w, h):
        raise MafError("eval_batch: batch shape %s is smaller than the %d x %d loaded frame: the reference would resize twice (load_image, then "
                       "letterbox); not supported" % (list(batch_shape), h, w))
    ratio, pad = g["ret"]
    g["shapes"] = ((h0, w0), ((h * ratio / h0, w * ratio / w0), pad))
    g["load_hw"] = (h, w)
    return g


# ---------------------------------------------------------------- device

def _frame_list(frames):
    if torch.is_tensor(frames):
        if frames.dim() != 4:
            raise MafError("letterbox: a single tensor of frames is uint8 [B, h, w, 3]")
        frames = list(frames.unbind(0))
    frames = list(frames)
    if not frames:
        raise MafError("letterbox: no frames")
    for f in frames:
        if not torch.is_tensor(f) or not f.is_cuda:
            raise MafError("letterbox runs on the HIP path only: frames must be CUDA tensors (no CPU fallback)")
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
            raise MafError("letterbox: frames are uint8 [h, w, 3] tensors, got %s %s" % (f.dtype, tuple(f.shape)))
        if f.stride(2) != 1 or f.stride(1) != 3:
            raise MafError("letterbox: a frame needs pixel stride 3 and channel stride 1 (rows may have any pitch)")
    return frames


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


def eval_batch(frames, img_size=640, stride=32, pad=0.5, shape=None, bgr=True):
    """The evaluation loader's batch (load_image + rect letterbox + collate_fn) from decoded frames -> (imgs uint8 [B, 3, H, W], shapes): the
    batch shape is `shape` ([H, W]) or the sort_files_shapes rule over this batch's aspect ratios; `shapes` is the per-image tuple that
    EvalLoop / convert_to_coco_format consume."""
    frames = _frame_list(frames)
    hw0 = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
    bs = list(shape) if shape is not None else rect_batch_shape(hw0, img_size, stride, pad)
    geoms = [eval_geometry(h0, w0, bs, img_size) for h0, w0 in hw0]
    H, W = geoms[0]["shape"]
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


def _upload(arr, dev):
    """Host array -> device on the current stream, without a host sync (pinned staging)."""
    return torch.from_numpy(arr).pin_memory().to(dev, non_blocking=True)


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
    cnt = _upload(np.array([int(o.shape[0]) for o in dets], np.int32), dev)
    _rescale(rows, cnt, letterboxed_hw, src_shapes, round)
    for b, o in enumerate(dets):
        o[:, :4] = rows[b, :o.shape[0], :4]
    return dets


def _rescale(rows, cnt, letterboxed_hw, src_shapes, do_round):
    B, max_det, stride = rows.shape
    if len(src_shapes) != B:
        raise MafError("rescale_boxes: %d source shapes for %d images" % (len(src_shapes), B))
    par = _upload(rescale_params(letterboxed_hw, src_shapes), rows.device)
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
