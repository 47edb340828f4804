"""The rule book of the BMP encoder (maf-yolo_amd/bmp_encode.py, csrc/bmp_encode.hip) in plain Python and numpy.  No GPU, no Pillow.

  * pixel_array(bgr)   the rows from the bottom one up, B, G, R per pixel, each padded with zeros to a multiple of 4 bytes;
  * header(w, h)       BITMAPFILEHEADER (BM, the file size, 0, 0, the pixel offset 54) and BITMAPINFOHEADER (40, w, h, planes 1, bit count 24,
                       compression 0 and five DWORDs of 0, the image size among them);
  * encode(bgr)        the file.
"""
import struct

import numpy as np

HEAD_BYTES = 54
FIELDS = ("magic", "file_size", "reserved1", "reserved2", "pixel_offset", "header_size", "width", "height", "planes", "bit_count", "compression",
          "image_size", "x_pixels_per_metre", "y_pixels_per_metre", "colours_used", "colours_important")
LAYOUT = "<2sIHHIIiiHHIIiiII"


def row_stride(w):
    return (3 * w + 3) // 4 * 4


def pixel_array(bgr):
    h, w = bgr.shape[:2]
    rows = np.zeros((h, row_stride(w)), np.uint8)
    rows[:, :3 * w] = bgr[::-1].reshape(h, 3 * w)
    return rows.tobytes()


def header(w, h):
    return struct.pack(LAYOUT, b"BM", HEAD_BYTES + row_stride(w) * h, 0, 0, HEAD_BYTES, 40, w, h, 1, 24, 0, 0, 0, 0, 0, 0)


def read_header(data):
    """The 54 header bytes of a file -> {field: value}."""
    return dict(zip(FIELDS, struct.unpack(LAYOUT, bytes(data[:HEAD_BYTES]))))


def encode(bgr):
    """uint8 [h, w, 3] BGR -> the BMP file (bytes)."""
    return header(bgr.shape[1], bgr.shape[0]) + pixel_array(bgr)
