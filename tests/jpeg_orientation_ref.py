"""The rule book of jpeg.decode(..., apply_orientation=True) in plain NumPy: the EXIF orientation (tag 0x0112 of IFD0, TIFF 6.0 / Exif 2.3) as
a permutation of the decoded pixels, behind tests/jpeg_ref.py (baseline) or tests/jpeg_progressive_ref.py (progressive).

With the stored grid src [h, w] the frame cv2.imread returns is
    1      dst[y, x] = src[y, x]                       [h, w]
    2      dst[y, x] = src[y, w - 1 - x]               [h, w]     mirrored left-right
    3      dst[y, x] = src[h - 1 - y, w - 1 - x]       [h, w]     turned by 180 degrees
    4      dst[y, x] = src[h - 1 - y, x]               [h, w]     mirrored top-bottom
    5      dst[y, x] = src[x, y]                       [w, h]     transposed
    6      dst[y, x] = src[h - 1 - x, y]               [w, h]     turned clockwise by 90 degrees
    7      dst[y, x] = src[h - 1 - x, w - 1 - y]       [w, h]     transposed along the other diagonal
    8      dst[y, x] = src[x, w - 1 - y]               [w, h]     turned counter-clockwise by 90 degrees
The judge is PIL.ImageOps.exif_transpose (tools/make_golden_jpeg_orientation.py stores its frames), not this table.
"""
import numpy as np

import jpeg_progressive_ref as PR
import jpeg_ref as R
from maf_yolo_amd import jpeg as J

SOURCE = {1: lambda y, x, h, w: (y, x), 2: lambda y, x, h, w: (y, w - 1 - x), 3: lambda y, x, h, w: (h - 1 - y, w - 1 - x),
          4: lambda y, x, h, w: (h - 1 - y, x), 5: lambda y, x, h, w: (x, y), 6: lambda y, x, h, w: (h - 1 - x, y),
          7: lambda y, x, h, w: (h - 1 - x, w - 1 - y), 8: lambda y, x, h, w: (x, w - 1 - y)}


def orient(src, orientation):
    """src uint8 [h, w, 3] -> the frame of that orientation ([w, h, 3] for 5 to 8), pixel by pixel from the table."""
    h, w = src.shape[:2]
    H, W = (w, h) if orientation >= 5 else (h, w)
    y, x = np.mgrid[0:H, 0:W]
    sy, sx = SOURCE[orientation](y, x, h, w)
    return np.ascontiguousarray(src[sy, sx])


def decode(data):
    """A baseline or progressive file -> the frame cv2.imread returns (uint8 BGR), its EXIF orientation applied."""
    info = J.parse(data, progressive=True)
    stored = PR.decode(data) if info.scans is not None else R.decode(data)
    return orient(stored, info.orientation or 1)
