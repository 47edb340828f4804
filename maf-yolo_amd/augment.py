"""Training batches augmented on the device: mosaic, random affine, mixup, HSV and flips ("device data augmentation").

The reference builds every training sample on the host with OpenCV, in TrainValDataset.__getitem__ (yolov6/data/datasets.py:147-275):
load_image resizes, mosaic_augmentation fills a 2s x 2s canvas, random_affine warps it to s x s, a cached second mosaic is mixed in for
images with few labels, augment_hsv and the flips follow (yolov6/data/data_augment.py).  Here:
  * TrainAugment(labels, shapes, hyp, img_size)   the host half: draws every random parameter of a sample from Python's `random` and NumPy's
                           `np.random` in the reference's exact order (same seeds, same batch as the reference dataset with num_workers = 0) and
                           computes the sample's final labels with the reference's own formulas and NumPy dtypes;
  * train_batch(frames, indices, aug)   __getitem__ x B + collate_fn: the load_image resizes (one launch, csrc/augment.hip maf_augment_resize)
                           and ONE launch of maf_mosaic_affine write the uint8 [B, 3, s, s] batch; the [N, 6] targets go up in one
                           non-blocking copy.  No device -> host synchronisation.

Scope.  Box labels by default: with no polygon segments the reference's copy_paste and mask_refine do nothing and draw nothing (copy_paste
only calls random.sample when a segment exists), and polygon segments raise MafError.  TrainAugment(..., segments, polygons=True) takes
YOLO-segment labels (one polygon per label row): copy_paste (data_augment.py:285-307) then picks objects with random.sample in the
reference's order, appends their mirrored boxes and polygons and records the int32 contours it hands to cv2.drawContours (Layer.paste);
random_affine(mask_refine=True) warps every polygon resampled to 1000 points and boxes it with segment2box.  On the device the contours
become one bit mask per layer (csrc/polygon_mask.hip maf_polygon_mask, OpenCV's FILLED rule as restated in tests/copy_paste_ref.py) and
maf_mosaic_affine_paste reads canvas (C-1-x, y) instead of (x, y) where the mask is set at (C-1-x, y), C = 2s.  The reference indexes
segments by label row and misindexes on datasets that mix box and polygon rows; here every image needs one polygon per row, or none.
`mixup > 1` reaches a call with the wrong signature in the reference (mixup(self, ..., type="simple")) and raises MafError.  albument, rect training and the per-worker RNG
streams of a multi-worker DataLoader are out of scope; frames arrive decoded, as uint8 HWC (BGR, cv2.imread order) CUDA tensors.

Labels keep the dtype the dataset gives them (TrainValDataset.labels are float32 arrays): every step below runs the reference's NumPy
expression on the same operand types (Python ints and floats where the reference has them), so the labels are bit-identical to what the
reference computes (tests/golden/augment_cases.npz).  The HSV lookup tables are computed in float64 exactly as augment_hsv does.
The pixels follow the rules of tests/augment_ref.py bit for bit (OpenCV's fixed-point warpAffine and uint8 HSV conversions, restated).
"""
import ctypes as C
import math
import random
from dataclasses import dataclass, field

import numpy as np
import torch

from . import lib, staging
from .letterbox import letterbox_geometry
from .lib import MafError

MAX_CACHED_IMAGES = 20          # TrainValDataset(max_cached_images=20, random_pop=False): the dynamic-mixup cache of get_cache_mosaic


@dataclass
class Tile:
    """One source image placed on the (virtual) canvas: canvas pixels [x0, x1) x [y0, y1) read frame pixel (x + dx, y + dy) of `frame`.
    frame: ("load", i) = image i after load_image, ("lb", i, nw, nh) = that image resized again by letterbox (non-mosaic branch only)."""
    frame: tuple
    hw: tuple                   # (h, w) of `frame`
    x0: int
    y0: int
    x1: int
    y1: int
    dx: int
    dy: int


@dataclass
class Layer:
    """One warped image: its tiles on the canvas, the affine matrix M (3 x 3, canvas -> output) and the scale s it was drawn with."""
    tiles: list
    M: np.ndarray
    s: float
    center: tuple = None        # mosaic centre (xc, yc); None in the non-mosaic branch
    paste: list = field(default_factory=list)   # copy_paste: the int32 [k, 2] contours handed to cv2.drawContours(FILLED), in order


@dataclass
class Sample:
    """Everything one __getitem__ drew, and its labels: [n, 5] (cls, x, y, w, h normalised), the reference's dtype."""
    index: int
    mosaic: bool
    layers: list                # [A] or [A, B] (B: the cached mosaic mixed in)
    mix_r: float = None         # mixup ratio of A (np.random.beta(32, 32)) when len(layers) == 2
    gains: np.ndarray = None    # HSV gains, None when hsv_h = hsv_s = hsv_v = 0 (no conversion, no draw)
    lut: np.ndarray = None      # uint8 [3, 256]: hue, saturation, value
    flipud: bool = False
    fliplr: bool = False
    labels: np.ndarray = field(default=None)


def rotation_matrix_2d(angle, scale):
    """cv2.getRotationMatrix2D(center=(0, 0), angle, scale) in closed form (double): [[a, b, 0], [-b, a, 0]], a = s cos, b = s sin."""
    t = angle * (math.pi / 180)                               # angle *= CV_PI / 180
    a, b = math.cos(t) * scale, math.sin(t) * scale
    cx = cy = 0.0
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]])


def invert_affine(M):
    """cv2.invertAffineTransform of M[:2] (the inversion warpAffine does without WARP_INVERSE_MAP), same operation order -> 6 doubles."""
    m = [float(v) for v in np.asarray(M, np.float64)[:2].reshape(-1)]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m[4] * D, m[0] * D
    m[0] = a11
    m[1] *= -D
    m[3] *= -D
    m[4] = a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def hsv_luts(gains):
    """augment_hsv's tables (data_augment.py:34-50) for gains r (float64 [3]) -> uint8 [3, 256]."""
    x = np.arange(0, 256, dtype=gains.dtype)
    return np.stack([((x * gains[0]) % 180).astype(np.uint8),
                     np.clip(x * gains[1], 0, 255).astype(np.uint8),
                     np.clip(x * gains[2], 0, 255).astype(np.uint8)])


class TrainAugment:
    """The host half of the training-time augmentation of TrainValDataset (augment=True, rect=False, dy_cache_mixup=True).

    labels  per image an [n, 5] array (cls, x, y, w, h normalised), as TrainValDataset.labels (float32 there)
    shapes  per image (h0, w0), the decoded frame's size
    hyp     the reference's data_aug dict (configs/MAF-YOLO-n.py:31-47): hsv_h/s/v, degrees, translate, scale, shear, flipud, fliplr,
            mosaic, mixup, dy_label, dy_mixup, copy_paste, mask_refine
    segments  optional per-image polygon lists.  polygons=False (the default): any non-empty one raises MafError (box labels only).
              polygons=True: segments[i] is a list of float [k, 2] arrays (normalised xy), one per row of labels[i] (an empty list for an
              image without labels), as the reference's label reader builds them from YOLO-segment files (datasets.py:746-749); draw then
              runs copy_paste and mask_refine as the reference does and Layer.paste holds the pasted contours

    draw(index) consumes `random` and `np.random` in the reference's order and returns a Sample.  The dynamic-mixup cache of
    get_cache_mosaic (max 20 entries, oldest popped, refilled with 3 random images while it holds <= 4) lives in the object, as it lives
    in the dataset: draws of one object form one stream."""

    def __init__(self, labels, shapes, hyp, img_size=640, segments=None, polygons=False):
        self.labels = list(labels)
        self.shapes = [(int(h), int(w)) for h, w in shapes]
        if len(self.labels) != len(self.shapes) or not self.labels:
            raise MafError("TrainAugment: one labels array and one (h0, w0) per image, at least one image")
        for lab in self.labels:
            if lab.ndim != 2 or lab.shape[1] != 5:
                raise MafError("TrainAugment: labels are [n, 5] (cls, x, y, w, h) box arrays; polygon labels are not supported")
        self.polygons = bool(polygons)
        if not self.polygons:
            if segments is not None and any(len(s) for s in segments):
                raise MafError("TrainAugment: polygon segments are not supported without polygons=True (box labels only: copy_paste / "
                               "mask_refine need segments)")
            self.segments = [[] for _ in self.labels]
        else:
            segments = [[] for _ in self.labels] if segments is None else [[np.asarray(x) for x in s] for s in segments]
            if len(segments) != len(self.labels):
                raise MafError("TrainAugment: one polygon list per image")
            for i, (lab, segs) in enumerate(zip(self.labels, segments)):
                if len(segs) != len(lab):
                    raise MafError("TrainAugment: image %d has %d polygons for %d label rows (polygons=True needs one polygon per row; "
                                   "datasets that mix box and polygon rows are not supported)" % (i, len(segs), len(lab)))
                for x in segs:
                    if x.ndim != 2 or x.shape[1] != 2 or not len(x) or x.dtype.kind != "f":
                        raise MafError("TrainAugment: a polygon is a float [k, 2] array of normalised xy with k >= 1")
            self.segments = segments
        self.hyp = dict(hyp)
        for k in ("test_load_size", "letterbox_return_int"):
            if k in self.hyp:
                raise MafError("TrainAugment: hyp[%r] is not supported" % k)
        if self.hyp["mixup"] > 1:
            raise MafError("TrainAugment: mixup > 1 reaches the reference's broken 'simple' mixup call (datasets.py:181-192); not supported")
        self.img_size = int(img_size)
        self.cache = []

    def __len__(self):
        return len(self.labels)

    def loaded_hw(self, i):
        """load_image (datasets.py:277-300) in augment mode, without the pixels: r = s / max(h0, w0) -> (int(h0 r), int(w0 r))."""
        h0, w0 = self.shapes[i]
        r = self.img_size / max(h0, w0)
        if r != 1:
            return int(h0 * r), int(w0 * r)
        return h0, w0

    # ---------------------------------------------------------------- the draws of __getitem__

    def draw(self, index):
        hyp, s = self.hyp, self.img_size
        if random.random() < hyp["mosaic"]:
            idx = [index] + random.choices(range(0, len(self)), k=3)
            random.shuffle(idx)
            layer, labels = self._mosaic([(i, self.loaded_hw(i), self.labels[i], self.segments[i]) for i in idx])
            sample = Sample(index, True, [layer])
            if random.random() < hyp["mixup"]:
                sample.labels = self._mixup(sample, labels, random.randint(0, len(self) - 1))
            elif len(labels) <= hyp["dy_label"] and random.random() < hyp["dy_mixup"]:
                sample.labels = self._mixup(sample, labels, random.randint(0, len(self) - 1))
            else:
                sample.labels = labels
            if random.random() < hyp["mixup"] - 1:                   # always drawn; unreachable with mixup <= 1 (checked in __init__)
                raise MafError("TrainAugment: the reference's 'simple' mixup branch is not supported")
        else:
            sample = self._letterboxed(index)
        labels = sample.labels
        if len(labels):
            h = w = s
            labels[:, [1, 3]] = labels[:, [1, 3]].clip(0, w - 1e-3)
            labels[:, [2, 4]] = labels[:, [2, 4]].clip(0, h - 1e-3)
            boxes = np.copy(labels[:, 1:])
            boxes[:, 0] = ((labels[:, 1] + labels[:, 3]) / 2) / w
            boxes[:, 1] = ((labels[:, 2] + labels[:, 4]) / 2) / h
            boxes[:, 2] = (labels[:, 3] - labels[:, 1]) / w
            boxes[:, 3] = (labels[:, 4] - labels[:, 2]) / h
            labels[:, 1:] = boxes
        # general_augment (datasets.py:642-668)
        nl = len(labels)
        if hyp["hsv_h"] or hyp["hsv_s"] or hyp["hsv_v"]:
            sample.gains = np.random.uniform(-1, 1, 3) * [hyp["hsv_h"], hyp["hsv_s"], hyp["hsv_v"]] + 1
            sample.lut = hsv_luts(sample.gains)
        if random.random() < hyp["flipud"]:
            sample.flipud = True
            if nl:
                labels[:, 2] = 1 - labels[:, 2]
        if random.random() < hyp["fliplr"]:
            sample.fliplr = True
            if nl:
                labels[:, 1] = 1 - labels[:, 1]
        sample.labels = labels
        return sample

    def draw_batch(self, indices):
        return [self.draw(int(i)) for i in indices]

    def _mixup(self, sample, labels, index):
        layer, labels2 = self._cache_mosaic(index)
        sample.layers.append(layer)
        sample.mix_r = np.random.beta(32.0, 32.0)
        return np.concatenate((labels, labels2), 0)

    def _cache_mosaic(self, index):
        """get_cache_mosaic (datasets.py:522-575): append, refill (<= 4) or pop the oldest (> 20), then the newest + 3 random entries."""
        self.cache.append((index, self.loaded_hw(index), self.labels[index], self.segments[index]))
        if len(self.cache) <= 4:
            idx = random.choices(range(0, len(self)), k=3)
            random.shuffle(idx)
            for i in idx:
                self.cache.append((i, self.loaded_hw(i), self.labels[i], self.segments[i]))
        elif len(self.cache) > MAX_CACHED_IMAGES:
            self.cache.pop(0)
        picks = [-1] + random.choices(range(0, len(self.cache) - 1), k=3)
        return self._mosaic([self.cache[p] for p in picks])

    def _mosaic(self, items):
        """mosaic_augmentation (data_augment.py:190-254) on (index, (h, w), labels, polygons) x 4 -> (Layer, labels after random_affine)."""
        s = self.img_size
        yc, xc = (int(random.uniform(s // 2, 3 * s // 2)) for _ in range(2))
        tiles, labels4, segment4 = [], [], []
        for k, (i, (h, w), lab, segs) in enumerate(items):
            if k == 0:
                x1a, y1a, x2a, y2a = max(xc - w, 0), max(yc - h, 0), xc, yc
                x1b, y1b = w - (x2a - x1a), h - (y2a - y1a)
            elif k == 1:
                x1a, y1a, x2a, y2a = xc, max(yc - h, 0), min(xc + w, s * 2), yc
                x1b, y1b = 0, h - (y2a - y1a)
            elif k == 2:
                x1a, y1a, x2a, y2a = max(xc - w, 0), yc, xc, min(s * 2, yc + h)
                x1b, y1b = w - (x2a - x1a), 0
            else:
                x1a, y1a, x2a, y2a = xc, yc, min(xc + w, s * 2), min(s * 2, yc + h)
                x1b, y1b = 0, 0
            tiles.append(Tile(("load", i), (h, w), x1a, y1a, x2a, y2a, x1b - x1a, y1b - y1a))
            padw, padh = x1a - x1b, y1a - y1b
            lab = lab.copy()
            if lab.size:
                boxes = np.copy(lab[:, 1:])
                boxes[:, 0] = w * (lab[:, 1] - lab[:, 3] / 2) + padw
                boxes[:, 1] = h * (lab[:, 2] - lab[:, 4] / 2) + padh
                boxes[:, 2] = w * (lab[:, 1] + lab[:, 3] / 2) + padw
                boxes[:, 3] = h * (lab[:, 2] + lab[:, 4] / 2) + padh
                lab[:, 1:] = boxes
                segs = [_xyn2xy(x, w, h, padw, padh) for x in segs]
            labels4.append(lab)
            segment4.extend(segs)
        labels4 = np.concatenate(labels4, 0)
        for x in (labels4[:, 1:], *segment4):
            np.clip(x, 0, 2 * s, out=x)
        paste = []
        if self.polygons and self.hyp["copy_paste"]:
            labels4, paste = _copy_paste(2 * s, labels4, segment4, self.hyp["copy_paste"])
        M, sc, labels4 = self._affine((2 * s, 2 * s), labels4, segment4)
        if not (M != np.eye(3)).any():
            raise MafError("TrainAugment: an identity transform on a mosaic (translate >= 0.5) returns the 2s canvas in the reference")
        return Layer(tiles, M, sc, (xc, yc), paste), labels4

    def _letterboxed(self, index):
        """The non-mosaic branch (datasets.py:194-237): load_image -> letterbox(auto=False, scaleup=True) -> random_affine."""
        s = self.img_size
        h, w = self.loaded_hw(index)
        g = letterbox_geometry(h, w, (s, s), auto=False, scaleup=True)
        ratio, pad = g["ret"]
        nw, nh = g["new_unpad"]
        frame = ("load", index) if (nw, nh) == (w, h) else ("lb", index, nw, nh)
        tile = Tile(frame, (nh, nw), g["left"], g["top"], g["left"] + nw, g["top"] + nh, -g["left"], -g["top"])
        labels = self.labels[index].copy()
        if labels.size:
            w *= ratio
            h *= ratio
            boxes = np.copy(labels[:, 1:])
            boxes[:, 0] = w * (labels[:, 1] - labels[:, 3] / 2) + pad[0]
            boxes[:, 1] = h * (labels[:, 2] - labels[:, 4] / 2) + pad[1]
            boxes[:, 2] = w * (labels[:, 1] + labels[:, 3] / 2) + pad[0]
            boxes[:, 3] = h * (labels[:, 2] + labels[:, 4] / 2) + pad[1]
            labels[:, 1:] = boxes
        M, sc, labels = self._affine((s, s), labels)
        sample = Sample(index, False, [Layer([tile], M, sc)])
        sample.labels = labels
        return sample

    def _affine(self, img_hw, labels, segments=()):
        """get_transform_matrix + random_affine (data_augment.py:111-187): six uniform draws; boxes from the corners -> min / max, clipped to
        the output, or, with polygons and mask_refine, from every polygon resampled to 1000 points, warped and boxed by segment2box; then
        box_candidates -> (M, s, labels)."""
        hyp, s = self.hyp, self.img_size
        height = width = s
        C = np.eye(3)
        C[0, 2] = -img_hw[1] / 2
        C[1, 2] = -img_hw[0] / 2
        R = np.eye(3)
        a = random.uniform(-hyp["degrees"], hyp["degrees"])
        sc = random.uniform(1 - hyp["scale"], 1 + hyp["scale"])
        R[:2] = rotation_matrix_2d(a, sc)
        S = np.eye(3)
        S[0, 1] = math.tan(random.uniform(-hyp["shear"], hyp["shear"]) * math.pi / 180)
        S[1, 0] = math.tan(random.uniform(-hyp["shear"], hyp["shear"]) * math.pi / 180)
        T = np.eye(3)
        T[0, 2] = random.uniform(0.5 - hyp["translate"], 0.5 + hyp["translate"]) * width
        T[1, 2] = random.uniform(0.5 - hyp["translate"], 0.5 + hyp["translate"]) * height
        M = T @ S @ R @ C
        n = len(labels)
        if n and any(x.any() for x in segments) and hyp["mask_refine"]:
            new = np.zeros((n, 4))
            for i, segment in enumerate(_resample_segments(segments)):
                xy = np.ones((len(segment), 3))
                xy[:, :2] = segment
                xy = xy @ M.T
                new[i] = _segment2box(xy[:, :2], width, height)
        elif n:
            xy = np.ones((n * 4, 3))
            xy[:, :2] = labels[:, [1, 2, 3, 4, 1, 4, 3, 2]].reshape(n * 4, 2)       # corners x1y1, x2y2, x1y2, x2y1
            xy = (xy @ M.T)[:, :2].reshape(n, 8)
            x, y = xy[:, [0, 2, 4, 6]], xy[:, [1, 3, 5, 7]]
            new = np.concatenate((x.min(1), y.min(1), x.max(1), y.max(1))).reshape(4, n).T
            new[:, [0, 2]] = new[:, [0, 2]].clip(0, width)
            new[:, [1, 3]] = new[:, [1, 3]].clip(0, height)
        if n:
            keep = _box_candidates(labels[:, 1:5].T * sc, new.T)
            labels = labels[keep]
            labels[:, 1:5] = new[keep]
        return M, sc, labels


def _xyn2xy(x, w, h, padw, padh):
    """xyn2xy (data_augment.py:279-284): a normalised polygon to canvas pixels, in the polygon's dtype."""
    y = np.copy(x)
    y[..., 0] = w * x[..., 0] + padw
    y[..., 1] = h * x[..., 1] + padh
    return y


def _bbox_ioa(box1, box2, eps=1e-7):
    """bbox_ioa (data_augment.py:308-327): intersection over the area of box2, [n, m]."""
    b1_x1, b1_y1, b1_x2, b1_y2 = box1.T
    b2_x1, b2_y1, b2_x2, b2_y2 = box2.T
    inter_area = (np.minimum(b1_x2[:, None], b2_x2) - np.maximum(b1_x1[:, None], b2_x1)).clip(0) * \
                 (np.minimum(b1_y2[:, None], b2_y2) - np.maximum(b1_y1[:, None], b2_y1)).clip(0)
    box2_area = (b2_x2 - b2_x1) * (b2_y2 - b2_y1) + eps
    return inter_area / box2_area


def _copy_paste(w, labels, segments, p):
    """copy_paste (data_augment.py:285-307) without the pixels: the objects whose mirror image overlaps every object by < 30 % are
    candidates, random.sample picks round(p n) of them (Python's round: half to even); each pick appends its mirrored label row and
    polygon (to `segments`, in place) and is drawn UNMIRRORED, truncated to int32 -> (labels, the contours in drawing order).
    w: the canvas width (2s), a Python int as im.shape gives it."""
    paste = []
    n = len(segments)
    if p and n:
        boxes = np.stack([w - labels[:, 3], labels[:, 2], w - labels[:, 1], labels[:, 4]], axis=-1)
        ioa = _bbox_ioa(boxes, labels[:, 1:5])
        indexes = np.nonzero((ioa < 0.30).all(1))[0]
        n = len(indexes)
        for j in random.sample(list(indexes), k=round(p * n)):
            l, box, s = labels[j], boxes[j], segments[j]
            labels = np.concatenate((labels, [[l[0], *box]]), 0)
            segments.append(np.concatenate((w - s[:, 0:1], s[:, 1:2]), 1))
            paste.append(segments[j].astype(np.int32))
    return labels, paste


def _resample_segments(segments, n=1000):
    """resample_segments (data_augment.py:328-335): every closed polygon to n points by linear interpolation over the vertex index."""
    out = []
    for s in segments:
        s = np.concatenate((s, s[0:1, :]), axis=0)
        x = np.linspace(0, len(s) - 1, n)
        xp = np.arange(len(s))
        out.append(np.concatenate([np.interp(x, xp, s[:, i]) for i in range(2)]).reshape(2, -1).T)
    return out


def _segment2box(segment, width, height):
    """segment2box (data_augment.py:336-341): the box of the points inside the image; np.zeros((1, 4)) when no inside point has a
    nonzero x (Python's any(x) on the x coordinates, as the reference writes it)."""
    x, y = segment.T
    inside = (x >= 0) & (y >= 0) & (x <= width) & (y <= height)
    x, y, = x[inside], y[inside]
    return np.array([x.min(), y.min(), x.max(), y.max()]) if any(x) else np.zeros((1, 4))


def _box_candidates(box1, box2, wh_thr=2, ar_thr=20, area_thr=0.1, eps=1e-16):
    """box_candidates (data_augment.py:99-105): kept when wider and taller than 2 px, > 10 % of the scaled area, aspect < 20."""
    w1, h1 = box1[2] - box1[0], box1[3] - box1[1]
    w2, h2 = box2[2] - box2[0], box2[3] - box2[1]
    ar = np.maximum(w2 / (h2 + eps), h2 / (w2 + eps))
    return (w2 > wh_thr) & (h2 > wh_thr) & (w2 * h2 / (w1 * h1 + eps) > area_thr) & (ar < ar_thr)


# ---------------------------------------------------------------- device

def needed_frames(samples):
    """The image indices a list of Samples reads (mosaic tiles, cached mosaics): what a trainer decodes for this batch."""
    return sorted({t.frame[1] for smp in samples for layer in smp.layers for t in layer.tiles})


def _check_frame(f, i, hw0):
    if not torch.is_tensor(f) or not f.is_cuda:
        raise MafError("train_batch runs on the HIP path only: frames must be CUDA tensors (no CPU fallback)")
    if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.stride(2) != 1 or f.stride(1) != 3:
        raise MafError("train_batch: frame %d must be uint8 [h, w, 3] with pixel stride 3 and channel stride 1 (rows may have any pitch), got "
                       "%s %s" % (i, f.dtype, tuple(f.shape)))
    if (int(f.shape[0]), int(f.shape[1])) != hw0:
        raise MafError("train_batch: frame %d is %d x %d, TrainAugment.shapes says %d x %d" % (i, f.shape[0], f.shape[1], hw0[0], hw0[1]))


def _pitch(f):
    return int(f.stride(0)) if f.shape[0] > 1 else 3 * int(f.shape[1])


def train_batch(frames, indices, aug):
    """TrainValDataset.__getitem__ for every index + collate_fn, on the device -> (imgs uint8 [B, 3, s, s] RGB, targets fp32 [N, 6]
    (image position in the batch, cls, x, y, w, h)), both on the frames' device.

    frames   indexable by dataset image index (a list, or a dict holding at least needed_frames(samples)): uint8 [h0, w0, 3] BGR CUDA tensors,
             views with any row pitch welcome, of the sizes aug.shapes gives
    indices  the batch's dataset indices (draws them with aug.draw, consuming `random` / `np.random`), or Samples drawn already
    aug      the TrainAugment holding the labels, hyp and the dynamic-mixup cache

    Two launches: the load_image resizes of every distinct frame the batch reads (plus letterbox's second resize where the non-mosaic branch
    takes one) into one staging buffer, then maf_mosaic_affine.  Tables and targets go up from pinned memory: no device -> host sync.
    When copy_paste pasted something in any layer of the batch (TrainAugment(polygons=True)), the contours go up with the sample table, one
    maf_polygon_mask launch draws every pasted layer's mask and maf_mosaic_affine_paste takes maf_mosaic_affine's place."""
    from . import torch_ops
    samples = [i if isinstance(i, Sample) else aug.draw(int(i)) for i in indices]
    if not samples:
        raise MafError("train_batch: no indices")
    host, dev, keep = stage_batch(frames, samples, aug)
    paste = stage_paste(samples)
    if paste is None:
        imgs = torch_ops.load().mosaic_affine(host, staging.upload(host.numpy(), dev), aug.img_size)
    else:
        imgs = _mosaic_affine_paste(host, paste, dev, aug.img_size)
    del keep                                                   # staging and resize tables: stream-ordered frees, after the launch
    n = sum(len(smp.labels) for smp in samples)
    targets = np.zeros((n, 6), np.float32)
    row = 0
    for b, smp in enumerate(samples):
        k = len(smp.labels)
        targets[row:row + k, 0] = b
        targets[row:row + k, 1:] = smp.labels
        row += k
    return imgs, staging.upload(targets, dev)


def stage_paste(samples):
    """The contours copy_paste drew for a batch -> None when no layer has any, else (the int32 table of maf_polygon_mask: mask_start |
    poly_start | xy, (n, npoly, nvert), [(sample, layer)] of each mask): one mask per layer with pasted contours."""
    slots = [(b, l) for b, smp in enumerate(samples) for l, layer in enumerate(smp.layers) if layer.paste]
    if not slots:
        return None
    polys = [np.ascontiguousarray(c, np.int32).reshape(-1, 2) for b, l in slots for c in samples[b].layers[l].paste]
    for c in polys:
        if not len(c) or np.abs(c).max() > lib.POLYGON_COORD_MAX:
            raise MafError("train_batch: a pasted contour needs a vertex, and coordinates within +-%d" % lib.POLYGON_COORD_MAX)
    mask_start = np.cumsum([0] + [len(samples[b].layers[l].paste) for b, l in slots])
    poly_start = np.cumsum([0] + [len(c) for c in polys])
    table = np.concatenate([mask_start, poly_start, np.concatenate(polys, 0).reshape(-1)]).astype(np.int32)
    return table, (len(slots), len(polys), int(poly_start[-1])), slots


def _mosaic_affine_paste(host, paste, dev, s):
    """maf_polygon_mask + maf_mosaic_affine_paste for a staged batch (host: stage_batch's sample table, paste: stage_paste's result).  The
    masks come from the caching allocator (the kernel writes every word: no memset); the sample table, the paste table and the contours go
    up in ONE copy from pinned memory."""
    from . import torch_ops
    table, (n, npoly, nvert), slots = paste
    B, side = host.shape[0], 2 * s
    words = side * ((side + 31) // 32)
    masks = torch.empty((n, words), dtype=torch.int32, device=dev)
    ptab = (lib.MafAugmentPaste * B)()
    for e in ptab:
        e.C = side
    for i, (b, l) in enumerate(slots):
        ptab[b].mask[l] = masks.data_ptr() + 4 * words * i
    parts = [host.numpy().reshape(-1), np.frombuffer(ptab, np.uint8), table.view(np.uint8)]
    offs = np.cumsum([0] + [(len(p) + 7) // 8 * 8 for p in parts])          # every part 8-byte aligned in the upload
    buf = np.zeros(int(offs[-1]), np.uint8)
    for o, p in zip(offs, parts):
        buf[o:o + len(p)] = p
    up = staging.upload(buf, dev)
    samples_dev, paste_dev, table_dev = (up[o:o + len(p)] for o, p in zip(offs, parts))
    st = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):                               # the C-ABI launches on the current device: the frames' one
        lib.check(lib.load().maf_polygon_mask(table.ctypes.data, table_dev.data_ptr(), n, npoly, nvert, side, masks.data_ptr(), st))
    paste_host = torch.from_numpy(parts[1].reshape(B, -1).copy())
    return torch_ops.load().mosaic_affine_paste(host, samples_dev.view(B, -1), paste_host, paste_dev.view(B, -1), s)


def stage_batch(frames, samples, aug):
    """The resize stage of train_batch (launched on the current stream) and the host table of maf_mosaic_affine -> (CPU uint8 [B, sizeof
    maf_augment_sample_t] table, device, buffers the table points into, to be kept until the mosaic_affine launch is queued)."""
    src = {}                                                   # frame key -> (tensor or None, ptr, pitch, h, w)
    resizes = [[], []]                                         # pass 0: load_image; pass 1: letterbox's second resize (reads pass 0)
    dev, staged = None, 0
    for key in sorted({t.frame for smp in samples for layer in smp.layers for t in layer.tiles}, key=lambda k: (len(k), k)):
        i = key[1]
        f = frames[i]
        _check_frame(f, i, aug.shapes[i])
        if dev is None:
            dev = f.device
        elif f.device != dev:
            raise MafError("train_batch: frames on one device")
        lkey = ("load", i)
        if lkey not in src:
            h, w = aug.loaded_hw(i)
            if (h, w) == aug.shapes[i]:
                src[lkey] = (f, f.data_ptr(), _pitch(f), h, w)
            else:
                src[lkey] = (None, staged, 3 * w, h, w)
                resizes[0].append((f.data_ptr(), _pitch(f), aug.shapes[i], lkey))
                staged += 3 * h * w
        if key[0] == "lb":
            nw, nh = key[2], key[3]
            src[key] = (None, staged, 3 * nw, nh, nw)
            resizes[1].append((lkey, nh, nw, key))
            staged += 3 * nh * nw
    stage = torch.empty(max(staged, 1), dtype=torch.uint8, device=dev)
    base = stage.data_ptr()

    def where(key):
        t, p, pitch, h, w = src[key]
        return (p if t is not None else base + p), pitch, h, w
    L = lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    tabs = []
    for k, items in enumerate(resizes):
        if not items:
            continue
        tab = (lib.MafAugmentFrame * len(items))()
        for e, item in zip(tab, items):
            if k == 0:
                ptr, pitch, (h0, w0), key = item
                e.src, e.src_pitch, e.h, e.w = ptr, pitch, h0, w0
            else:
                lkey, nh, nw, key = item
                e.src, e.src_pitch, e.h, e.w = where(lkey)
            e.dst = where(key)[0]
            e.new_h, e.new_w = src[key][3], src[key][4]
        host = np.frombuffer(tab, np.uint8).copy()
        tab_dev = staging.upload(host, dev)
        tabs.append(tab_dev)
        lib.check(L.maf_augment_resize(C.addressof(tab), tab_dev.data_ptr(), len(items), st))
    table = (lib.MafAugmentSample * len(samples))()
    for e, smp in zip(table, samples):
        for l, layer in enumerate(smp.layers):
            e.minv[l][:] = invert_affine(layer.M)
            e.ntiles[l] = len(layer.tiles)
            for k, t in enumerate(layer.tiles):
                d = e.tile[l][k]
                d.ptr, d.pitch, d.h, d.w = where(t.frame)
                d.x0, d.y0, d.x1, d.y1, d.dx, d.dy = t.x0, t.y0, t.x1, t.y1, t.dx, t.dy
        e.r = float(smp.mix_r) if smp.mix_r is not None else 0.0
        e.flipud, e.fliplr = int(smp.flipud), int(smp.fliplr)
        if smp.lut is not None:
            e.hsv = 1
            np.frombuffer(e.lut, np.uint8)[:] = np.ascontiguousarray(smp.lut, np.uint8).reshape(-1)
    host = torch.from_numpy(np.frombuffer(table, np.uint8).reshape(len(samples), -1).copy())
    return host, dev, (stage, tabs)
