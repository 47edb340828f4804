"""NumPy restatement of the pixels of the reference's copy_paste (yolov6/data/data_augment.py:285-307): the mask cv2.drawContours(im_new,
[contour], -1, (1, 1, 1), cv2.FILLED) draws, and im[flip(im_new) != 0] = flip(im)[...] on the mosaic canvas.

OpenCV is not a dependency of this project, so the fill rule is pinned here, restated from OpenCV's drawing code (imgproc/drawing.cpp:
drawContours with thickness < 0 -> CollectPolyEdges + FillEdgeCollection, i.e. fillPoly with line_type 8 and shift 0; Line -> LineIterator;
clipLine).  The HIP kernel (maf-yolo_amd/csrc/polygon_mask.hip) must equal this restatement bit for bit, and the tests hold it to that.
Agreement with one particular OpenCV build is unpinned by construction (releases differ in how CollectPolyEdges treats edges that leave the
image); tests/test_copy_paste_host.py bounds how far the rule can be from the true polygon: away from the edges it equals an exact
even-odd point-in-polygon test and Pillow's polygon fill.

Rules, for one contour v[0..n-1] of int32 vertices (they may lie outside the C x C canvas) — the mask is the union of (a) and (b), and the
mask of several contours is the union of theirs:
  (a) Outline.  Every edge v[i-1] -> v[i] (i = 0 closes the contour from v[n-1]; horizontal and zero-length edges included) is drawn as
      cv::LineIterator(img, p1, p2, 8, leftToRight=true) visits it:
        * clipLine to [0, C-1]^2 first (it moves the endpoints): codes c = (x < 0) + 2 (x > C-1) + 4 (y < 0) + 8 (y > C-1); nothing is
          drawn when c1 & c2 != 0 after either stage; a point above / below moves to y = 0 / C-1 with x += (a - y)(x2 - x1) / (y2 - y1),
          then a point left / right moves to x = 0 / C-1 with y += (a - x)(y2 - y1) / (x2 - x1), each quotient truncated towards zero
          (OpenCV computes it in double and casts to int64: for |coordinates| <= 32767 that equals the truncating integer division, as
          |quotient| <= 65534 while a double resolves 2^-36 there and a non-integer quotient is at least 2^-17 from an integer), and the
          second point's move uses the first point's moved coordinates;
        * dx = x2 - x1, dy = y2 - y1; dx < 0 -> start from p2 (dx, dy negated); the major axis is y when |dy| > |dx|; with D, d the major
          and minor lengths: err = D - 2 d, D + 1 pixels from the start; before each step, err < 0 -> one minor step and err += 2 D; every
          step moves one along the major axis and err -= 2 d.
  (b) Interior (FillEdgeCollection).  Every non-horizontal edge, upper vertex (x0, y0), lower (x1, y1): x = x0 << 16 (16.16 fixed point),
      step = ((x1 - x0) << 16) / (y1 - y0) truncated towards zero, active on rows y0 <= y < y1 with x(y) = (x0 << 16) + (y - y0) step.
      On every row 0 <= y < C the active x, sorted, are paired; a pair (xl, xr) fills columns (xl + 65535) >> 16 .. xr >> 16, clipped to
      [0, C-1].  (OpenCV keeps the active edges sorted by x and walks them in pairs, so only the sorted values matter.)  Equivalently —
      the form the kernel uses — column c is filled iff the number of active x < (c << 16) is odd, or some active x == (c << 16).
"""
import numpy as np

import augment_ref as R

COORD_MAX = 32767                  # MAF_POLYGON_COORD_MAX: |vertex coordinate| the C-ABI accepts


def _tdiv(p, q):
    """C++ integer division: truncated towards zero."""
    a = abs(p) // abs(q)
    return a if (p < 0) == (q < 0) else -a


def clip_line(C, x1, y1, x2, y2):
    """cv::clipLine(Size(C, C), p1, p2) -> the moved endpoints, or None when nothing of the segment is inside."""
    right = bottom = C - 1
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += _tdiv((a - y1) * (x2 - x1), y2 - y1)
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += _tdiv((a - y2) * (x2 - x1), y2 - y1)
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += _tdiv((a - x1) * (y2 - y1), x2 - x1)
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += _tdiv((a - x2) * (y2 - y1), x2 - x1)
                x2 = a
                c2 = 0
    return (x1, y1, x2, y2) if (c1 | c2) == 0 else None


def line_pixels(C, p1, p2):
    """The pixels cv::LineIterator(img, p1, p2, 8, true) visits on a C x C image, in order."""
    ends = clip_line(C, int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1]))
    if ends is None:
        return []
    x1, y1, x2, y2 = ends
    dx, dy = x2 - x1, y2 - y1
    sx = sy = 1
    if dx < 0:
        dx, dy, x1, y1 = -dx, -dy, x2, y2
    if dy < 0:
        dy, sy = -dy, -1
    vert = dy > dx
    D, d = (dy, dx) if vert else (dx, dy)
    err = D - 2 * d
    x, y, out = x1, y1, []
    for _ in range(D + 1):
        out.append((x, y))
        minor = err < 0
        err += -2 * d + (2 * D if minor else 0)
        if vert:
            y += sy
            x += sx if minor else 0
        else:
            x += sx
            y += sy if minor else 0
    return out


def fill_one(poly, C):
    """One contour (int [n, 2], n >= 1) -> bool [C, C], True where drawContours(..., FILLED) writes."""
    v = [(int(x), int(y)) for x, y in np.asarray(poly).reshape(-1, 2)]
    mask = np.zeros((C, C), bool)
    toggles = np.zeros((C, C + 1), np.int64)
    for i in range(len(v)):
        p0, p1 = v[i - 1], v[i]
        for x, y in line_pixels(C, p0, p1):
            mask[y, x] = True
        if p0[1] == p1[1]:
            continue
        (x0, y0), (x1, y1) = (p0, p1) if p0[1] < p1[1] else (p1, p0)
        step = _tdiv((x1 - x0) << 16, y1 - y0)
        for y in range(max(y0, 0), min(y1, C)):
            x = (x0 << 16) + (y - y0) * step
            c = x >> 16                                         # floor
            if (x & 0xFFFF) == 0 and 0 <= c < C:
                mask[y, c] = True
            toggles[y, min(max(c + 1, 0), C)] += 1              # columns c' with (c' << 16) > x see one more active x below them
    return mask | ((np.cumsum(toggles, 1)[:, :C] & 1) == 1)


def fill_mask(polys, C):
    """The union mask of the contours drawn one by one into a zero image: bool [C, C]."""
    mask = np.zeros((C, C), bool)
    for p in polys:
        mask |= fill_one(p, C)
    return mask


def pack_bits(mask):
    """bool [C, C] -> uint32 [C, ceil(C / 32)], pixel x of a row in bit x & 31 of word x >> 5: the layout of maf_polygon_mask."""
    C = mask.shape[1]
    W = (C + 31) // 32
    m = np.zeros((mask.shape[0], W * 32), np.uint64)
    m[:, :C] = mask
    return (m.reshape(mask.shape[0], W, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def polygon_table(masks):
    """A list of masks, each a list of int [k, 2] contours -> the int32 table of maf_polygon_mask and (n, npoly, nvert):
    mask_start [n + 1] | poly_start [npoly + 1] | xy [2 nvert]."""
    polys = [np.asarray(p, np.int32).reshape(-1, 2) for m in masks for p in m]
    mask_start = np.cumsum([0] + [len(m) for m in masks])
    poly_start = np.cumsum([0] + [len(p) for p in polys])
    xy = np.concatenate(polys + [np.zeros((0, 2), np.int32)], 0).reshape(-1)
    return np.concatenate([mask_start, poly_start, xy]).astype(np.int32), (len(masks), len(polys), int(poly_start[-1]))


def paste_canvas(canvas, mask):
    """im[flip(im_new) != 0] = flip(im)[...]: pixel (x, y) becomes the original (C-1-x, y) wherever the mask is set at (C-1-x, y)."""
    return np.where(mask[:, ::-1, None], canvas[:, ::-1], canvas)


def layer_pixels(aug, layer, frames, paste=True):
    """One warped layer of a Sample -> uint8 [s, s, 3] BGR; the mosaic canvas is materialised, pasted, then warped by augment_ref's rule."""
    from maf_yolo_amd.augment import invert_affine
    s = aug.img_size
    tiles = [R.RefTile(frames[t.frame], t.x0, t.y0, t.x1, t.y1, t.dx, t.dy) for t in layer.tiles]
    if paste and layer.paste:
        C = 2 * s
        canvas = paste_canvas(R.canvas_of(tiles, C)[1:-1, 1:-1], fill_mask(layer.paste, C))
        tiles = [R.RefTile(canvas, 0, 0, C, C, 0, 0)]
    return R.warp_canvas(tiles, invert_affine(layer.M), s)


def sample_pixels(aug, smp, frames, paste=True):
    """One Sample of maf_yolo_amd.augment (polygons=True) -> uint8 [3, s, s] RGB, what __getitem__ returns as its image;
    paste=False renders the same draws without copy_paste's pixels."""
    imgs = [layer_pixels(aug, layer, frames, paste) for layer in smp.layers]
    img = imgs[0] if len(imgs) == 1 else R.blend(imgs[0], imgs[1], smp.mix_r)
    if smp.lut is not None:
        img = R.hsv_augment(img, smp.lut)
    img = R.flip(img, smp.flipud, smp.fliplr)
    return np.ascontiguousarray(img.transpose(2, 0, 1)[::-1])
