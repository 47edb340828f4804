"""NumPy restatement of the pixels of the reference's letterbox (yolov6/data/data_augment.py:53-82: cv2.resize INTER_LINEAR, then
cv2.copyMakeBorder BORDER_CONSTANT) and of precess_image's HWC -> CHW, BGR -> RGB (yolov6/core/inferer.py:169-179).

OpenCV is not a dependency of this project, so the rule is pinned here, from OpenCV's uint8 INTER_LINEAR (imgproc/resize.cpp); the HIP kernel
(maf-yolo_amd/csrc/letterbox.hip) must equal this restatement bit for bit, and the tests hold it to that.  Agreement with one particular
OpenCV build is unpinned by construction (like torchvision.ops.nms for the NMS): expect at most 1 LSB of difference on some pixels.

Rules, for a source of w x h resized to nw x nh (cv2.resize(im, (nw, nh))):
  * Column coefficients.  scale_x = 1 / (nw / w) in double.  fx = float((dx + 0.5) * scale_x - 0.5) (double arithmetic, rounded to float),
    sx = floor(fx), fx -= sx (float).  Clamp: sx < 0 -> sx = 0, fx = 0; sx >= w - 1 -> sx = w - 1, fx = 0.
  * Row coefficients.  The same sequence with scale_y = 1 / (nh / h), BUT without the coefficient clamp: OpenCV's resize computes the
    vertical weights from the unclamped fy and clamps only the row index (rows clip(sy, 0, h - 1) and clip(sy + 1, 0, h - 1)).  At the top
    edge of an upscale (sy = -1) both rows are row 0 and the weights stay (1 - fy, fy).
  * Fixed point.  Each coefficient c in {1 - f, f} becomes saturate_cast<short>(c * 2048): c * 2048 in float, rounded half to even on its own
    (a0 + a1 need not be 2048).
  * Horizontal pass in int32: S = src[sx] * a0 + src[sx + 1] * a1 per channel (a1 = 0 at a clamped column).
  * Vertical pass: the rounding of OpenCV's vector path (VResizeLinearVec_32s8u): out = (((S0 >> 4) * b0 >> 16) + ((S1 >> 4) * b1 >> 16) + 2) >> 2,
    saturated to uint8.  OpenCV's scalar tail, used for the last (row bytes mod vector width) bytes of a row, rounds as
    (S0 * b0 + S1 * b1 + 2^21) >> 22 instead, which can differ by 1; this restatement uses the vector form for every byte.
  * An exact 2x downscale on both axes (w = 2 nw and h = 2 nh) takes OpenCV's area-fast path: (a + b + c + d + 2) >> 2 over the 2 x 2 block
    (the 1280 x 720 -> 640 x 360 case).  Equal sizes: no resize (letterbox skips cv2.resize), a copy.
  * Border: the constant `color` per channel, in the frame's channel order (copyMakeBorder's value), around the unpadded image at (top, left).
  * Output: uint8 [3, H, W] with RGB planes; BGR input (cv2.imread) is swapped as precess_image's [::-1] does; bgr=False takes RGB frames.
"""
import numpy as np


def _coef(n_dst, n_src, clamp):
    scale = 1.0 / (float(n_dst) / float(n_src))
    d = np.arange(n_dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp:
        lo = s < 0
        s[lo], f[lo] = 0, 0
        hi = s >= n_src - 1
        s[hi], f[hi] = n_src - 1, 0
    c0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, c0, c1


def resize_linear(src, nw, nh):
    """cv2.resize(src, (nw, nh), interpolation=cv2.INTER_LINEAR) for uint8 [h, w, C], by the rules of the module docstring."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    if (w, h) == (nw, nh):
        return src.copy()
    s = src.astype(np.int64)
    if w == 2 * nw and h == 2 * nh:
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    sx, a0, a1 = _coef(nw, w, True)
    sx1 = np.minimum(sx + 1, w - 1)
    hor = s[:, sx] * a0[None, :, None] + s[:, sx1] * a1[None, :, None]                 # [h, nw, C] int32 range
    sy, b0, b1 = _coef(nh, h, False)
    r0, r1 = np.clip(sy, 0, h - 1), np.clip(sy + 1, 0, h - 1)
    S0, S1 = hor[r0], hor[r1]
    out = ((((S0 >> 4) * b0[:, None, None]) >> 16) + (((S1 >> 4) * b1[:, None, None]) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def letterbox_pixels(frame, new_unpad, top, left, H, W, color=(114, 114, 114), bgr=True):
    """One frame uint8 [h, w, 3] -> uint8 [3, H, W] RGB: resize to new_unpad = (nw, nh), border `color`, channel swap when bgr."""
    nw, nh = new_unpad
    im = resize_linear(frame, nw, nh)
    canvas = np.empty((H, W, 3), np.uint8)
    canvas[:] = np.asarray(color, np.uint8)
    canvas[top:top + nh, left:left + nw] = im
    chw = canvas.transpose(2, 0, 1)
    return np.ascontiguousarray(chw[::-1] if bgr else chw)


def rescale(letterboxed_hw, boxes, src_hw, do_round=True):
    """Inferer.rescale (inferer.py:181-195) + .round(): ratio and padding in double, then per coordinate in fp32 (x - pad) / ratio (an IEEE
    divide: torch's CPU operation order), clamp to the frame, round half to even.  boxes: fp32 [n, >= 4] array, columns 0..3 rewritten."""
    H, W = letterboxed_hw
    h0, w0 = src_hw
    ratio = min(H / h0, W / w0)
    px, py = np.float32((W - w0 * ratio) / 2), np.float32((H - h0 * ratio) / 2)
    b = np.array(boxes, np.float32)
    b[:, [0, 2]] = np.clip((b[:, [0, 2]] - px) / np.float32(ratio), np.float32(0), np.float32(w0))
    b[:, [1, 3]] = np.clip((b[:, [1, 3]] - py) / np.float32(ratio), np.float32(0), np.float32(h0))
    if do_round:
        b[:, :4] = np.rint(b[:, :4])
    return b


def synth_frame(h, w, seed):
    """A deterministic uint8 [h, w, 3] frame with gradients, edges and noise (every pixel value in play)."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 7) % 256], -1)
    noise = rs.randint(0, 256, (h, w, 3))
    return np.where(rs.rand(h, w, 1) < 0.3, noise, base).astype(np.uint8)

