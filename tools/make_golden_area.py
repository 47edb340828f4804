"""Golden vectors for the INTER_AREA evaluation path: the reference's OWN loader code run here, in the build container, on
batches of frame sizes — TrainValDataset.__getitem__ in evaluation mode (yolov6/data/datasets.py:197-215: load_image with
hyp["test_load_size"], then letterbox with hyp["letterbox_return_int"]) and sort_files_shapes (:670-695) for the rect batches.

    python tools/make_golden_area.py        ->  tests/golden/area_cases.npz

cv2 is stubbed as in tools/make_golden_letterbox.py: resize records (dsize, interpolation) and returns an array of that size, which is all
the geometry needs.  The fixture holds geometry only; the pixel rule is restated in tests/area_ref.py and the frames of the tests come from
letterbox_ref.synth_frame.

  cases [n, 7]  float64: case, img_size, test_load_size, rect, pad (force_no_pad: 0.0), letterbox_return_int, frames
  rows  [m, 20] float64, one per frame in the order given: case, h0, w0, loaded h, w, load_image's resize calls (0 / 1), its interpolation
                (cv2.INTER_LINEAR = 1, cv2.INTER_AREA = 3, -1 without a call), batch shape H, W, letterbox's new_unpad w, h, letterbox's
                resize calls, top, left, then `shapes`: h0, w0 again, ratio h, ratio w, pad[0], pad[1]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_letterbox as G  # noqa: E402

# (frames [(h0, w0), ...], img_size, test_load_size, rect, pad, letterbox_return_int)
REPRO = [(480, 640), (640, 480), (640, 640), (427, 640), (640, 427), (500, 375), (375, 500), (333, 500), (612, 612), (640, 359), (1080, 1920),
         (720, 1280), (640, 3), (1041, 800), (700, 1069)]    # 1041 at 638 and 1069 at 630: int(w0 * r) lands one below the load size
CASES = [
    (REPRO, 640, 638, False, 0.0, True),                       # configs/experiment/eval_640_repro.py, default / MAFYOLOs
    (REPRO, 640, 630, False, 0.0, True),                       # MAFYOLOm
    ([(48, 64), (64, 43), (64, 64)], 64, 62, False, 0.0, True),
    ([(48, 64), (64, 43), (64, 64), (30, 40)], 64, 63, False, 0.0, False),
    ([(200, 300), (96, 128), (150, 180), (64, 100), (1080, 1920), (128, 128)], 128, 128, True, 0.5, False),
    ([(300, 200), (128, 96), (180, 150), (100, 64), (480, 270)], 128, 128, True, 0.0, True),
    ([(200, 300), (300, 200), (128, 128), (131, 257)], 128, 128, True, 0.5, False),
    ([(400, 300), (200, 320), (640, 640), (161, 97)], 128, 160, False, 0.0, True),        # test_load_size above img_size: letterbox shrinks again
    ([(1080, 1920), (720, 1280), (1080, 1440), (2160, 3840)], 640, 640, True, 0.5, False),
    ([(480, 640), (427, 640), (375, 500)], 320, 320, True, 0.5, False),
    ([(480, 640), (640, 480), (500, 333)], 416, 416, False, 0.5, False),
]


def main():
    letterbox, DS, _, _ = G.load_reference()
    cases, rows = [], []
    for ci, (frames, img_size, load_size, rect, pad, ret_int) in enumerate(CASES):
        paths = ["%d_%d.jpg" % (ci, k) for k in range(len(frames))]
        for p, s in zip(paths, frames):
            G.IMREAD[p] = s
        self = DS.__new__(DS)
        self.__dict__.update(img_paths=list(paths), labels=[np.zeros((0, 5), np.float32) for _ in frames], augment=False, albument=False,
                             hyp=dict(test_load_size=load_size, letterbox_return_int=ret_int), rect=rect, img_size=img_size, stride=32, pad=pad,
                             shapes=np.array([[w, h] for h, w in frames], np.float64), batch_indices=np.zeros(len(frames), np.int64))
        if rect:
            DS.sort_files_shapes(self)                        # sorts img_paths by aspect ratio, sets batch_shapes
        for p, (h0, w0) in zip(paths, frames):
            G.CALLS.clear()
            img, _, path, shapes = DS.__getitem__(self, self.img_paths.index(p))
            assert path == p and shapes[0] == (h0, w0)
            rz = [c for c in G.CALLS if c[0] == "resize"]
            (top, bottom, left, right) = [c for c in G.CALLS if c[0] == "border"][0][1]
            r = load_size / max(h0, w0)
            load = rz[:1] if r != 1 else []                   # load_image resizes exactly when r != 1; a later call is letterbox's
            lb = rz[len(load):]
            h, w = (load[0][1][1], load[0][1][0]) if load else (h0, w0)
            nu = lb[0][1] if lb else (w, h)
            assert len(lb) <= 1 and (not lb or lb[0][2] == 1)
            H, W = int(img.shape[1]), int(img.shape[2])
            assert (H, W) == (nu[1] + top + bottom, nu[0] + left + right)
            rows.append([ci, h0, w0, h, w, len(load), load[0][2] if load else -1, H, W, nu[0], nu[1], len(lb), top, left,
                         shapes[0][0], shapes[0][1], shapes[1][0][0], shapes[1][0][1], float(shapes[1][1][0]), float(shapes[1][1][1])])
        cases.append([ci, img_size, load_size, int(rect), pad, int(ret_int), len(frames)])
    path = os.path.join(ROOT, "tests", "golden", "area_cases.npz")
    np.savez_compressed(path, cases=np.array(cases, np.float64), rows=np.array(rows, np.float64))
    rows = np.array(rows)
    print("wrote %s: %d cases, %d frames (%d INTER_AREA loads, %d second resizes)" % (path, len(cases), len(rows), int((rows[:, 6] == 3).sum()),
                                                                                      int(((rows[:, 6] == 3) & (rows[:, 11] == 1)).sum())))


if __name__ == "__main__":
    main()
