"""Golden vectors for the letterbox layer: the reference's OWN geometry code run here, in the build container, on seeded
frame sizes — letterbox() (yolov6/data/data_augment.py:53-82), TrainValDataset.load_image (yolov6/data/datasets.py:277-300) and
sort_files_shapes (:670-695) with a stand-in `self`, Inferer.rescale (yolov6/core/inferer.py:181-195) + .round() on the CPU.

    python tools/make_golden_letterbox.py        ->  tests/golden/letterbox_cases.npz

cv2 is stubbed: resize / copyMakeBorder / imread return arrays of the right shape (no pixels) and record their size arguments, which is all the
geometry needs; PIL, tqdm and the modules inferer.py imports for drawing and loading are stubbed too.  The pixel rule is restated in
tests/letterbox_ref.py."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_import  # noqa: E402

CALLS = []


def _resize(im, dsize, interpolation=None):
    CALLS.append(("resize", tuple(dsize), interpolation))
    return np.zeros((dsize[1], dsize[0]) + im.shape[2:], np.uint8)


def _border(im, top, bottom, left, right, border_type, value=None):
    CALLS.append(("border", (top, bottom, left, right), tuple(value) if value is not None else None))
    return np.zeros((im.shape[0] + top + bottom, im.shape[1] + left + right) + im.shape[2:], np.uint8)


IMREAD = {}


def load_reference():
    ref_import.load(lambda b, s, t: torch.zeros(0, dtype=torch.long))       # cv2 / torchvision / timm / addict stubs
    cv2 = sys.modules["cv2"]
    cv2.__dict__.update(resize=_resize, copyMakeBorder=_border, imread=lambda p: np.zeros(IMREAD[p] + (3,), np.uint8),
                        INTER_LINEAR=1, INTER_AREA=3, BORDER_CONSTANT=0)
    cv2.__getattr__ = lambda name: 0                         # drawing constants inferer.py reads at class level

    def stub(name, **attrs):
        if name not in sys.modules:
            m = types.ModuleType(name)
            sys.modules[name] = m
        sys.modules[name].__dict__.update(attrs)

    stub("PIL", ExifTags=types.SimpleNamespace(TAGS={}), Image=object, ImageOps=object, ImageFont=object)
    stub("PIL.ExifTags", TAGS={}); stub("PIL.Image"); stub("PIL.ImageOps"); stub("PIL.ImageFont")
    stub("tqdm", tqdm=lambda x, *a, **k: x)
    stub("albumentations")
    stub("yaml", safe_load=lambda *a, **k: {})
    stub("yolov6.data.datasets_new", LoadData=object)
    from yolov6.data.data_augment import letterbox
    from yolov6.data.datasets import TrainValDataset
    try:
        from yolov6.core.inferer import Inferer
        rescale, check = Inferer.rescale, Inferer.check_img_size
        print("Inferer imported from the reference")
    except Exception as e:                                   # noqa: BLE001
        raise SystemExit("yolov6.core.inferer does not import with the stubs (%r): extend the stubs" % e)
    return letterbox, TrainValDataset, rescale, check


def main():
    letterbox, DS, rescale, check_img_size = load_reference()
    rs = np.random.RandomState(2026)
    out = {}
    # ---- letterbox(): (h, w, new_h, new_w, auto, scaleup, stride) -> r, new_unpad, top, bottom, left, right, dw, dh, left/top (return_int), out shape
    sizes = [(1080, 1920), (720, 1280), (480, 640), (333, 500), (17, 1000), (1, 1), (1000, 17), (640, 640), (427, 640), (640, 427),
             (1, 5000), (5000, 1), (2, 3), (375, 500), (500, 375), (612, 612), (321, 643), (1281, 721), (240, 320), (3, 1920)]
    cases = []
    for h, w in sizes:
        for ns in (640, 320, (384, 640), 1280):
            for auto in (True, False):
                for scaleup in (True, False):
                    cases.append((h, w, ns, auto, scaleup, 32))
    while len(cases) < 600:
        h, w = int(rs.randint(1, 2200)), int(rs.randint(1, 2200))
        if rs.rand() < 0.3:                                  # exact .5 products: w * r = k + 0.5
            k = int(rs.randint(1, 700)); w = 2 * k + 1; h = int(rs.randint(1, 2 * w))
        ns = [int(rs.choice([320, 416, 640, 1280]))] * 2 if rs.rand() < 0.7 else [int(rs.choice([256, 384, 480])), int(rs.choice([512, 640]))]
        cases.append((h, w, tuple(ns), bool(rs.rand() < 0.5), bool(rs.rand() < 0.8), int(rs.choice([32, 64]))))
    rows = []
    for h, w, ns, auto, scaleup, stride in cases:
        im = np.zeros((h, w, 3), np.uint8)
        CALLS.clear()
        _, r, (dw, dh) = letterbox(im, ns, auto=auto, scaleup=scaleup, stride=stride)
        rz = [c for c in CALLS if c[0] == "resize"]
        (top, bottom, left, right) = [c for c in CALLS if c[0] == "border"][0][1]
        nu = rz[0][1] if rz else (w, h)
        _, _, (li, ti) = letterbox(im, ns, auto=auto, scaleup=scaleup, stride=stride, return_int=True)
        nsh, nsw = (ns, ns) if isinstance(ns, int) else ns
        rows.append([h, w, nsh, nsw, int(auto), int(scaleup), stride, r, nu[0], nu[1], top, bottom, left, right, float(dw), float(dh), li, ti,
                     1 if rz else 0])
    out["lb"] = np.array(rows, np.float64)
    # ---- Inferer.check_img_size
    class _Self:
        make_divisible = staticmethod(lambda x, d: int(np.ceil(x / d) * d))
    import io, contextlib
    cis = []
    for v in (640, 600, 1, 33, 1280, 321):
        with contextlib.redirect_stdout(io.StringIO()):
            cis.append([v, 32] + list(check_img_size(_Self(), v, 32)))
    out["check_img_size"] = np.array(cis, np.int64)
    # ---- load_image (evaluation: augment False) + sort_files_shapes for one batch + the rect letterbox of __getitem__ -> shapes
    ev = []
    batches = [[(480, 640), (333, 500), (640, 427), (375, 500)], [(427, 640), (480, 640)], [(640, 480), (500, 375), (640, 612)],
               [(640, 640)], [(17, 600), (1, 1)], [(500, 333), (640, 427)]]
    for _ in range(40):
        n = int(rs.randint(1, 9))
        bt = []
        for _ in range(n):
            m = int(rs.randint(1, 641)); o = int(rs.randint(1, m + 1))
            bt.append((m, o) if rs.rand() < 0.5 else (o, m))
        batches.append(bt)
    for bi, bt in enumerate(batches):
        for img_size in (640, 320) if bi < 6 else (640,):
            if max(max(s) for s in bt) > img_size:
                continue
            paths = ["%d_%d.jpg" % (bi, k) for k in range(len(bt))]
            for p, s in zip(paths, bt):
                IMREAD[p] = s
            self = types.SimpleNamespace(img_paths=list(paths), labels=[None] * len(bt), shapes=np.array([[w, h] for h, w in bt], np.float64),
                                         batch_indices=np.zeros(len(bt), np.int64), img_size=img_size, stride=32, pad=0.5, augment=False)
            DS.sort_files_shapes(self)                       # sorts self.img_paths by aspect ratio, sets batch_shapes
            bs = self.batch_shapes[0]
            for p in self.img_paths:
                CALLS.clear()
                img, (h0, w0), (h, w) = DS.load_image(self, self.img_paths.index(p))
                im2, ratio, pad = letterbox(img, bs, auto=False, scaleup=False)
                assert im2.shape[:2] == tuple(bs)
                rz = [c for c in CALLS if c[0] == "resize"]
                (top, bottom, left, right) = [c for c in CALLS if c[0] == "border"][0][1]
                shapes = (h0, w0), ((h * ratio / h0, w * ratio / w0), pad)
                ev.append([bi, img_size, h0, w0, h, w, int(bs[0]), int(bs[1]), top, left, len(rz), rz[0][2] if rz else -1,
                           shapes[1][0][0], shapes[1][0][1], shapes[1][1][0], shapes[1][1][1], ratio])
            out["eval_batch_%d_%d" % (bi, img_size)] = np.array([[h, w] for h, w in bt], np.int64)
    out["eval"] = np.array(ev, np.float64)
    # ---- Inferer.rescale(...).round() on seeded fp32 boxes, torch on the CPU
    g = torch.Generator().manual_seed(99)
    resc = []
    boxes_all, res_all = [], []
    for ci, ((H, W), (h0, w0)) in enumerate([((384, 640), (1080, 1920)), ((384, 640), (720, 1280)), ((480, 640), (480, 640)), ((640, 640), (333, 500)),
                                              ((32, 640), (17, 1000)), ((640, 640), (1, 1)), ((448, 640), (333, 500)), ((640, 384), (1920, 1080)),
                                              ((640, 640), (1000, 17)), ((352, 640), (321, 643))]):
        n = [0, 1, 7, 300, 33][ci % 5]
        b = torch.rand(n, 6, generator=g) * torch.tensor([W * 1.2, H * 1.2, W * 1.2, H * 1.2, 1.0, 80.0]) - torch.tensor([W * 0.1, H * 0.1, W * 0.1, H * 0.1, 0, 0])
        b[: n // 4, :4] = torch.round(b[: n // 4, :4] * 2) / 2                   # exact .5 coordinates
        det = b.clone()
        if n:
            det[:, :4] = rescale((H, W), det[:, :4], (h0, w0, 3)).round()
        boxes_all.append(b.numpy()); res_all.append(det.numpy())
        resc.append([H, W, h0, w0, n])
    out["rescale_meta"] = np.array(resc, np.int64)
    out["rescale_in"] = np.concatenate(boxes_all, 0).astype(np.float32)
    out["rescale_out"] = np.concatenate(res_all, 0).astype(np.float32)
    path = os.path.join(ROOT, "tests", "golden", "letterbox_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d letterbox cases, %d eval rows, %d rescale boxes" % (path, len(rows), len(ev), out["rescale_in"].shape[0]))


if __name__ == "__main__":
    main()
