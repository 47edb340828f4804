"""NumPy restatement of OpenCV's uint8 INTER_AREA shrink: cv2.resize(src, (nw, nh), interpolation=cv2.INTER_AREA) with 1 <= nw <= w and
1 <= nh <= h, the only case TrainValDataset.load_image (yolov6/data/datasets.py:277-300) reaches with r < 1 in evaluation.

OpenCV is not a dependency of this project, so the rule is pinned here, from OpenCV's imgproc/resize.cpp (resize(), ResizeAreaFast_Invoker,
computeResizeAreaTab, ResizeArea_Invoker); the HIP kernel (maf-yolo_amd/csrc/resize_area.hip) must equal this restatement bit for bit, and
the tests hold it to that.  Agreement with one particular OpenCV build is unpinned by construction: a build whose compiler contracts
a * b + c into an FMA can differ by 1 LSB on pixels that sit on a rounding tie.  `import cv2` does not work where this file was written,
so the restatement could not be compared with cv2's own output, and tests/golden/area_cases.npz holds no cv2 pixels.

Rules, for a source of w x h resized to nw x nh:
  * Scale and path.  scale_x = 1.0 / (nw / w), scale_y = 1.0 / (nh / h), in double, in exactly this operation order.  iscale = scale rounded
    half to even.  The "fast" path is taken when abs(scale_x - iscale_x) < DBL_EPSILON and abs(scale_y - iscale_y) < DBL_EPSILON, computed
    in float64 as written (not w % nw == 0).
  * Fast path, iscale_x == iscale_y == 2: (a + b + c + d + 2) >> 2 over the 2 x 2 block (letterbox_ref.resize_linear's 2x rule).
  * Fast path, any other integer factors (1 x 1 included: a copy): the integer sum over the iscale_y x iscale_x block; float32(sum) times
    float32(1.0f / (iscale_x * iscale_y)) in float32; rounded half to even, clamped to 0..255.  With exact factors no partial cell arises
    (asserted: w == iscale_x * nw and h == iscale_y * nh).
  * General path, the decimation table of an axis (n_src -> n_dst, scale as above), in double.  For dx in 0 .. n_dst - 1:
    fsx1 = dx * scale; fsx2 = fsx1 + scale; cell = min(scale, n_src - fsx1); sx1 = ceil(fsx1); sx2 = min(floor(fsx2), n_src - 1);
    sx1 = min(sx1, sx2).  Entries of dx, in this order:
      if sx1 - fsx1 > 1e-3:            (sx1 - 1, float32((sx1 - fsx1) / cell))
      for sx in sx1 .. sx2 - 1:        (sx, float32(1.0 / cell))
      if fsx2 - sx2 > 1e-3:            (sx2, float32(min(min(fsx2 - sx2, 1.0), cell) / cell))
  * General path, accumulation, all in float32, every multiply and every add rounded on its own (no FMA), in resizeArea_'s order: for one
    destination pixel and channel walk the y-entries of its row in table order; for each source row buf = 0, then
    buf = buf + float32(S[sx]) * alpha_x over the x-entries of its column in table order; the first source row gives sum = beta * buf, later
    rows sum = sum + beta * buf.  Output: sum rounded half to even, clamped to 0..255.
"""
import math

import numpy as np

import letterbox_ref

DBL_EPSILON = 2.220446049250313e-16
F32 = np.float32


def scales(h, w, nh, nw):
    """-> (scale_x, scale_y, iscale_x, iscale_y, fast)."""
    scale_x, scale_y = 1.0 / (float(nw) / float(w)), 1.0 / (float(nh) / float(h))
    ix, iy = int(round(scale_x)), int(round(scale_y))                      # Python's round(): half to even
    return scale_x, scale_y, ix, iy, abs(scale_x - ix) < DBL_EPSILON and abs(scale_y - iy) < DBL_EPSILON


def area_tab(n_src, n_dst):
    """computeResizeAreaTab: one axis -> a list over dx of lists of (source index, float32 alpha)."""
    scale = 1.0 / (float(n_dst) / float(n_src))
    tab = []
    for dx in range(n_dst):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, n_src - fsx1)
        sx1, sx2 = math.ceil(fsx1), min(math.floor(fsx2), n_src - 1)
        sx1 = min(sx1, sx2)
        e = []
        if sx1 - fsx1 > 1e-3:
            e.append((sx1 - 1, F32((sx1 - fsx1) / cell)))
        for sx in range(sx1, sx2):
            e.append((sx, F32(1.0 / cell)))
        if fsx2 - sx2 > 1e-3:
            e.append((sx2, F32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
        tab.append(e)
    return tab


def _padded(tab):
    """A table as arrays [n_dst, K]: source index, alpha, valid (K = the most entries any index owns)."""
    K = max(len(e) for e in tab)
    si, al, ok = np.zeros((len(tab), K), np.int64), np.zeros((len(tab), K), F32), np.zeros((len(tab), K), bool)
    for d, e in enumerate(tab):
        for k, (s, a) in enumerate(e):
            si[d, k], al[d, k], ok[d, k] = s, a, True
    return si, al, ok


def _round_u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def resize_area_general(src, nw, nh):
    """The decimation-table path, whatever the factors (resize_area takes it when OpenCV does)."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    S = src.astype(F32)
    xsi, xal, xok = _padded(area_tab(w, nw))
    ysi, yal, yok = _padded(area_tab(h, nh))
    total = None
    for ky in range(ysi.shape[1]):                                         # vectorised over pixels, one step per tap
        rows = S[ysi[:, ky]]                                               # [nh, w, C]
        buf = np.zeros((nh, nw, S.shape[2]), F32)
        for kx in range(xsi.shape[1]):
            step = buf + rows[:, xsi[:, kx]] * xal[None, :, kx, None]      # float32 multiply, then float32 add: two roundings
            buf = np.where(xok[None, :, kx, None], step, buf)
        term = yal[:, ky, None, None] * buf
        if ky == 0:
            total = term                                                   # every index owns at least one entry
        else:
            total = np.where(yok[:, ky, None, None], total + term, total)
    assert xok[:, 0].all() and yok[:, 0].all() and total.dtype == F32
    return _round_u8(total)


def resize_area(src, nw, nh):
    """cv2.resize(src, (nw, nh), interpolation=cv2.INTER_AREA) for uint8 [h, w, C] with 1 <= nw <= w, 1 <= nh <= h, by the rules above."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    assert src.dtype == np.uint8 and 1 <= nw <= w and 1 <= nh <= h
    _, _, ix, iy, fast = scales(h, w, nh, nw)
    if not fast:
        return resize_area_general(src, nw, nh)
    assert w == ix * nw and h == iy * nh, "OpenCV's fast path with a partial cell"
    blocks = src.astype(np.int64).reshape(nh, iy, nw, ix, -1)
    total = blocks.sum(axis=(1, 3))
    if ix == 2 and iy == 2:
        return ((total + 2) >> 2).astype(np.uint8)
    return _round_u8(total.astype(F32) * (F32(1.0) / F32(ix * iy)))


def load_letterbox_pixels(frame, load_wh, new_unpad, top, left, H, W, color=(114, 114, 114), bgr=True):
    """load_image's INTER_AREA shrink to load_wh = (w, h), then letterbox(): INTER_LINEAR to new_unpad = (nw, nh) when the sizes still
    differ, border `color`, channel swap when bgr -> uint8 [3, H, W] RGB (letterbox_ref.letterbox_pixels does the second half)."""
    small = resize_area(frame, load_wh[0], load_wh[1])
    return letterbox_ref.letterbox_pixels(small, new_unpad, top, left, H, W, color, bgr)
