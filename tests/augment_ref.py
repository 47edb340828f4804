"""NumPy restatement of the pixels of the reference's training augmentation (yolov6/data/datasets.py:147-275 with
yolov6/data/data_augment.py): load_image's cv2.resize, the mosaic canvas, cv2.warpAffine, mixup, augment_hsv (cv2.cvtColor BGR <-> HSV,
cv2.LUT), the flips and the HWC -> CHW / BGR -> RGB of __getitem__.

OpenCV is not a dependency of this project, so the rules are pinned here, restated from OpenCV's uint8 code paths (imgproc/imgwarp.cpp
warpAffine + remap INTER_LINEAR, imgproc/color_hsv); the HIP kernels (maf-yolo_amd/csrc/augment.hip) must equal this restatement bit for
bit, and the tests hold them to that.  Agreement with one particular OpenCV build is unpinned by construction (OpenCV releases differ in
their SIMD paths; 4.11's new warp kernels compute coordinates in float): expect at most 1 LSB of difference on some pixels.

Rules:
  * Resize (load_image, augment mode): r = s / max(h0, w0); when r != 1, INTER_LINEAR to (int(w0 r), int(h0 r)), the rule of
    tests/letterbox_ref.py (resize_linear, exact-2x area-fast path included).  The non-mosaic branch letterboxes that image to s x s with
    auto=False, scaleup=True: when letterbox's new_unpad differs from the loaded size (a long side that load_image rounds to s - 1), a
    second INTER_LINEAR resize of the loaded image follows.
  * Canvas.  Never materialised by the kernel: a canvas pixel (x, y) lies in at most one tile rectangle [x0, x1) x [y0, y1) of
    mosaic_augmentation (data_augment.py:225-262) and reads frame pixel (x + dx, y + dy) there; everywhere else it is 114 (the canvas fill,
    and warpAffine's BORDER_CONSTANT value outside the 2s x 2s canvas: the same number, so the canvas size drops out).  The non-mosaic branch
    is one tile, the letterboxed image at (left, top) of an s x s canvas.
  * warpAffine (imgwarp.cpp WarpAffineInvoker + remapBilinear, uint8).  M is inverted as invertAffineTransform does
    (maf-yolo_amd/augment.py invert_affine) -> m[0..5].  INTER_BITS = 5, AB_BITS = 10, AB_SCALE = 1024, round_delta = 16:
      adelta[x] = rint(m0 * x * 1024), bdelta[x] = rint(m3 * x * 1024)                   (double, saturate_cast<int>: half to even)
      X0[y] = rint((m1 * y + m2) * 1024) + 16,  Y0[y] = rint((m4 * y + m5) * 1024) + 16
      X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;  sx = X >> 5, sy = Y >> 5 (saturated to int16), fx = X & 31, fy = Y & 31
      weights (32 x 32 table): (32 - fx)(32 - fy) 32, fx (32 - fy) 32, (32 - fx) fy 32, fx fy 32 — they sum to exactly 32768
      (OpenCV stores 32767 for fx = fy = 0 and normalises; a single tap of weight >= 32767 rounds to that tap either way)
      out = (v(sx, sy) w0 + v(sx + 1, sy) w1 + v(sx, sy + 1) w2 + v(sx + 1, sy + 1) w3 + (1 << 14)) >> 15, each neighbour from the canvas
    The reference skips warpAffine when M == I (data_augment.py:130); under this rule the identity warp is an exact copy, so the skip needs
    no case of its own.
  * Mixup (data_augment.py:86-97): (a * r + b * (1 - r)) in double, truncated to uint8 as astype(np.uint8) does; a = the sample's warped
    mosaic, b = the cached mosaic's.
  * HSV (augment_hsv, data_augment.py:34-50), when any gain is nonzero.  uint8 BGR2HSV (hsv_shift = 12, hue range 180):
      v = max(b, g, r), diff = v - min(b, g, r), sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)), sdiv[0] = hdiv[0] = 0
      s = (diff sdiv[v] + 2048) >> 12
      h = g - b if v == r else (b - r + 2 diff if v == g else r - g + 4 diff);  h = (h hdiv[diff] + 2048) >> 12;  h += 180 if h < 0
    then the three uint8 tables (computed on the host in float64 as augment_hsv does), then uint8 HSV2BGR in float32:
      h' = h * (6 / 180 as float), s' = s * (1 / 255 as float), v' = v; s' == 0 -> b = g = r = v'; else sector = floor(h'), f = h' - sector,
      tab = (v', v'(1 - s'), v'(1 - s' f), v'(1 - s'(1 - f))), (b, g, r) = tab[SECTOR[sector]], each rounded half to even and saturated.
  * Flips: flipud then fliplr, applied as an index map; then HWC -> CHW with the planes reversed (BGR -> RGB): uint8 [3, s, s].
"""
from dataclasses import dataclass

import numpy as np

from letterbox_ref import resize_linear, synth_frame  # noqa: F401

GREY = 114
SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


@dataclass
class RefTile:
    frame: np.ndarray            # uint8 [h, w, 3] BGR
    x0: int
    y0: int
    x1: int
    y1: int
    dx: int
    dy: int


def bilinear_table():
    """[fy, fx] -> the four fixed-point weights (top-left, top-right, bottom-left, bottom-right), int64 [32, 32, 4]."""
    f = np.arange(32)
    fy, fx = np.meshgrid(f, f, indexing="ij")
    return np.stack([(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32], -1).astype(np.int64)


def canvas_of(tiles, size):
    """The canvas, materialised (the spec may): [size + 2, size + 2, 3] with a ring of 114 around [0, size)."""
    c = np.full((size + 2, size + 2, 3), GREY, np.uint8)
    for t in tiles:
        c[t.y0 + 1:t.y1 + 1, t.x0 + 1:t.x1 + 1] = t.frame[t.y0 + t.dy:t.y1 + t.dy, t.x0 + t.dx:t.x1 + t.dx]
    return c


def warp_canvas(tiles, minv, s, canvas_size=None):
    """cv2.warpAffine(canvas, M, (s, s), borderValue=114) by the rules above; minv = invertAffineTransform(M) -> uint8 [s, s, 3]."""
    m = [float(v) for v in minv]
    size = canvas_size or max([2 * s] + [max(t.x1, t.y1) for t in tiles])
    c = canvas_of(tiles, size).astype(np.int64)
    xs = np.arange(s, dtype=np.float64)
    adelta = np.rint(m[0] * xs * 1024).astype(np.int64)
    bdelta = np.rint(m[3] * xs * 1024).astype(np.int64)
    X0 = np.rint((m[1] * xs + m[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((m[4] * xs + m[5]) * 1024).astype(np.int64) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    w = bilinear_table()[Y & 31, X & 31]

    def tap(x, y):                                    # the ring is 114, and so is everything a clip lands on outside [0, size)
        return c[np.clip(y + 1, 0, size + 1), np.clip(x + 1, 0, size + 1)]
    acc = (tap(sx, sy) * w[..., 0:1] + tap(sx + 1, sy) * w[..., 1:2] + tap(sx, sy + 1) * w[..., 2:3] + tap(sx + 1, sy + 1) * w[..., 3:4])
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def blend(a, b, r):
    return (a.astype(np.float64) * r + b.astype(np.float64) * (1 - r)).astype(np.uint8)


def _div_tables():
    i = np.arange(256, dtype=np.float64)
    with np.errstate(divide="ignore"):
        sdiv = np.where(i > 0, np.rint((255 << 12) / np.maximum(i, 1)), 0).astype(np.int64)
        hdiv = np.where(i > 0, np.rint((180 << 12) / (6.0 * np.maximum(i, 1))), 0).astype(np.int64)
    return sdiv, hdiv


def bgr2hsv(img):
    """cv2.cvtColor(img, COLOR_BGR2HSV) for uint8 -> (h, s, v) int64 arrays."""
    sdiv, hdiv = _div_tables()
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * sdiv[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def hsv2bgr(h, s, v):
    """cv2.cvtColor(hsv, COLOR_HSV2BGR) for uint8 (float32 arithmetic) -> uint8 [..., 3]."""
    f32 = np.float32
    hf = h.astype(f32) * f32(f32(6.0) / f32(180))
    sf = s.astype(f32) * f32(f32(1.0) / f32(255.0))
    vf = v.astype(f32)
    hf = np.fmod(hf, f32(6.0))
    sector = np.floor(hf).astype(np.int64)
    hf = (hf - sector.astype(f32)).astype(f32)
    bad = (sector < 0) | (sector >= 6)
    sector = np.where(bad, 0, sector)
    hf = np.where(bad, f32(0), hf).astype(f32)
    one = f32(1.0)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * hf), vf * (one - sf * (one - hf))], -1).astype(f32)
    bgr = np.take_along_axis(tab, SECTOR[sector], -1)
    bgr = np.where((sf == 0)[..., None], vf[..., None], bgr)
    return np.clip(np.rint(bgr), 0, 255).astype(np.uint8)


def hsv_augment(img, lut):
    """BGR2HSV -> the three tables (uint8 [3, 256]) -> HSV2BGR."""
    h, s, v = bgr2hsv(img)
    return hsv2bgr(lut[0][h].astype(np.int64), lut[1][s].astype(np.int64), lut[2][v].astype(np.int64))


def flip(img, ud, lr):
    if ud:
        img = img[::-1]
    if lr:
        img = img[:, ::-1]
    return img


def staged_frames(aug, samples, raw):
    """load_image (and letterbox's second resize) for every frame key the samples reference; raw: index -> uint8 [h0, w0, 3]."""
    out = {}
    for smp in samples:
        for layer in smp.layers:
            for t in layer.tiles:
                i = t.frame[1]
                h, w = aug.loaded_hw(i)
                key = ("load", i)
                if key not in out:
                    out[key] = resize_linear(raw[i], w, h) if (h, w) != raw[i].shape[:2] else raw[i]
                if t.frame[0] == "lb" and t.frame not in out:
                    out[t.frame] = resize_linear(out[key], t.frame[2], t.frame[3])
    return out


def sample_pixels(aug, smp, frames):
    """One Sample of maf_yolo_amd.augment -> uint8 [3, s, s] RGB, what __getitem__ returns as its image."""
    from maf_yolo_amd.augment import invert_affine
    s = aug.img_size
    imgs = []
    for layer in smp.layers:
        tiles = [RefTile(frames[t.frame], t.x0, t.y0, t.x1, t.y1, t.dx, t.dy) for t in layer.tiles]
        imgs.append(warp_canvas(tiles, invert_affine(layer.M), s))
    img = imgs[0] if len(imgs) == 1 else blend(imgs[0], imgs[1], smp.mix_r)
    if smp.lut is not None:
        img = hsv_augment(img, smp.lut)
    img = flip(img, smp.flipud, smp.fliplr)
    return np.ascontiguousarray(img.transpose(2, 0, 1)[::-1])
