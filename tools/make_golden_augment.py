"""Golden vectors for the training augmentation (maf-yolo_amd/augment.py): the reference's OWN TrainValDataset.__getitem__
(yolov6/data/datasets.py:147-275, with get_mosaic, get_cache_mosaic, mosaic_augmentation, random_affine, mixup, general_augment) run here,
in the build container, on a stand-in `self` (object.__new__) with seeded Python `random` and NumPy `np.random`.

    python tools/make_golden_augment.py        ->  tests/golden/augment_cases.npz

cv2 is stubbed: imread returns zeros of seeded shapes (the image index written into the first pixel, so that every later copy says which
image it is); resize, warpAffine, copyMakeBorder, cvtColor, split, LUT and merge return arrays of the right shape and record their
arguments; getRotationMatrix2D is restated in closed form.  albumentations, PIL and tqdm are stubbed.  Recorded per sample: the image
indices and loaded sizes of every mosaic tile, the mosaic centres, M and s of each random_affine, the mixup flag and ratio, the HSV gains
and tables, the flip flags and labels_out.  Three hyp sets: the MAF-YOLO-n defaults, mosaic = 0 (the last epochs) and dy_mixup = 1 with few
labels per image (mixup and the cache path on most samples).  Data only: nothing of the reference is stored."""
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ref_import  # noqa: E402

HYP_N = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, flipud=0.0, fliplr=0.5,
             mosaic=1.0, mixup=0.0, dy_label=5, dy_mixup=0.2, mask_refine=True, copy_paste=0.05)
SETS = {
    "default": (HYP_N, 12),
    "nomosaic": (dict(HYP_N, mosaic=0.0, mixup=0.0, dy_mixup=0.0), 12),
    "dymixup": (dict(HYP_N, dy_mixup=1.0, degrees=5.0, shear=2.0, flipud=0.5), 4),
}
DRAWS = 240
LOG = []


def _imread(path):
    i, h, w = (int(v) for v in os.path.basename(path).split(".")[0].split("_"))
    im = np.zeros((h, w, 3), np.uint8)
    im[0, 0, 0], im[0, 0, 1] = i & 255, i >> 8
    return im


def _tag(im):
    return int(im[0, 0, 0]) | int(im[0, 0, 1]) << 8


def _resize(im, dsize, interpolation=None):
    LOG.append(("resize", _tag(im), im.shape[:2], (dsize[1], dsize[0])))
    out = np.zeros((dsize[1], dsize[0], 3), np.uint8)
    out[0, 0, :2] = im[0, 0, :2]
    return out


def _border(im, top, bottom, left, right, border_type, value=None):
    LOG.append(("border", top, left))
    return np.zeros((im.shape[0] + top + bottom, im.shape[1] + left + right, 3), np.uint8)


def _warp(img, M, dsize, borderValue=None):
    LOG.append(("warp", np.array(M, np.float64)))
    return np.zeros((dsize[1], dsize[0], 3), np.uint8)


def _rotation(center, angle, scale):
    """cv2.getRotationMatrix2D's closed form (imgproc/imgwarp.cpp), double."""
    t = angle * (math.pi / 180)                               # angle *= CV_PI / 180
    a, b = math.cos(t) * scale, math.sin(t) * scale
    cx, cy = center
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]])


def _lut(ch, table):
    LOG.append(("lut", np.array(table, np.uint8)))
    return ch


def load_reference():
    ref_import.load(lambda b, s, t: torch.zeros(0, dtype=torch.long))       # cv2 / torchvision / timm / addict stubs
    cv2 = sys.modules["cv2"]
    cv2.__dict__.update(imread=_imread, resize=_resize, copyMakeBorder=_border, warpAffine=_warp, getRotationMatrix2D=_rotation,
                        cvtColor=lambda im, code, dst=None: np.zeros_like(im), split=lambda im: (im[..., 0], im[..., 1], im[..., 2]),
                        LUT=_lut, merge=lambda chs: np.stack(chs, -1), INTER_LINEAR=1, INTER_AREA=3, BORDER_CONSTANT=0,
                        COLOR_BGR2HSV=40, COLOR_HSV2BGR=54)
    cv2.__getattr__ = lambda name: 0

    def stub(name, **attrs):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
        sys.modules[name].__dict__.update(attrs)

    stub("PIL", ExifTags=types.SimpleNamespace(TAGS={}), Image=object, ImageOps=object, ImageFont=object)
    stub("PIL.ExifTags", TAGS={}); stub("PIL.Image"); stub("PIL.ImageOps"); stub("PIL.ImageFont")
    stub("tqdm", tqdm=lambda x, *a, **k: x)
    stub("albumentations")
    stub("yaml", safe_load=lambda *a, **k: {})
    from yolov6.data import data_augment, datasets
    return data_augment, datasets


def dataset(rs, n_img, max_labels):
    """Seeded image sizes (long sides that load_image rounds to 639, sizes above and below 640, exactly 640) and float32 box labels."""
    sizes = [(480, 640), (640, 640), (77, 60), (1080, 1920), (303, 200), (1, 1), (720, 1280), (638, 17), (1280, 1280), (333, 500)]
    while len(sizes) < n_img:
        a, b = int(rs.randint(16, 1400)), int(rs.randint(16, 1400))
        sizes.append((a, b))
    labels = []
    for _ in range(n_img):
        n = int(rs.randint(0, max_labels + 1))
        cxy = rs.uniform(0.05, 0.95, (n, 2))
        wh = rs.uniform(0.01, 0.6, (n, 2))
        labels.append(np.concatenate([rs.randint(0, 80, (n, 1)), cxy, wh], 1).astype(np.float32))
    return sizes, labels


def run_set(DA, DS, name, hyp, max_labels, seed):
    rs = np.random.RandomState(seed)
    sizes, labels = dataset(rs, 40, max_labels)
    self = object.__new__(DS.TrainValDataset)
    self.__dict__.update(augment=True, hyp=dict(hyp), img_size=640, rect=False, albument=False, dy_cache_mixup=True,
                         img_paths=["%d_%d_%d.jpg" % (i, h, w) for i, (h, w) in enumerate(sizes)], labels=labels,
                         segments=[np.zeros((0, 5), np.float32)] * len(sizes), all_results_cache=[], max_cached_images=20,
                         random_pop=False, num=0, num1=0, small_num=0)
    order = rs.randint(0, len(sizes), DRAWS)
    records = dict(int=[], tiles=[], M=[], s=[], r=[], gain=[], lut=[], labels=[])
    mos, tm = [], []
    real_mosaic, real_tm = DS.mosaic_augmentation, DA.get_transform_matrix

    def mosaic(img_size, imgs, hs, ws, labels, hyp, segments=None):
        state = DA.random.getstate()
        yc, xc = (int(DA.random.uniform(img_size // 2, 3 * img_size // 2)) for _ in range(2))     # the centre the call below draws
        DA.random.setstate(state)
        mos.append(([_tag(im) for im in imgs], list(zip(hs, ws)), (xc, yc)))
        return real_mosaic(img_size, imgs, hs, ws, labels, hyp, segments)

    def transform(*a, **k):
        M, s = real_tm(*a, **k)
        tm.append((np.array(M), s))
        return M, s

    real_beta, real_unif = np.random.beta, np.random.uniform
    got = {}
    np.random.beta = lambda *a: got.setdefault("r", real_beta(*a))
    np.random.uniform = lambda *a: got.setdefault("g", real_unif(*a))
    flips = []
    real_ud, real_lr = np.flipud, np.fliplr
    np.flipud = lambda m: (flips.append("ud"), real_ud(m))[1]
    np.fliplr = lambda m: (flips.append("lr"), real_lr(m))[1]
    DS.mosaic_augmentation, DA.get_transform_matrix = mosaic, transform
    import random
    random.seed(seed)
    np.random.seed(seed)
    try:
        for index in order:
            LOG.clear(); mos.clear(); tm.clear(); flips.clear(); got.clear()
            img, labels_out, _, _ = DS.TrainValDataset.__getitem__(self, int(index))
            assert tuple(img.shape) == (3, 640, 640)
            warps = [e for e in LOG if e[0] == "warp"]
            luts = [e[1] for e in LOG if e[0] == "lut"]
            tiles = np.full((8, 3), -1, np.int64)
            cen = [-1] * 4
            top = left = nw = nh = -1
            if mos:
                for k, (idx, hw, c) in enumerate(mos):
                    tiles[4 * k:4 * k + 4, 0] = idx
                    tiles[4 * k:4 * k + 4, 1:] = hw
                    cen[2 * k:2 * k + 2] = c
            else:
                h0, w0 = sizes[int(index)]
                rz = [e for e in LOG if e[0] == "resize"]
                h, w = rz[0][3] if rz and rz[0][2] == (h0, w0) else (h0, w0)
                tiles[0] = (int(index), h, w)
                lbz = [e for e in rz if e[2] == (h, w) and e[3] != (h, w)]
                nh, nw = lbz[-1][3] if lbz else (h, w)
                _, top, left = [e for e in LOG if e[0] == "border"][0]
            Ms = np.zeros((2, 3, 3)); ss = np.zeros(2)
            for k, (M, s) in enumerate(tm):
                Ms[k], ss[k] = M, s
            mixup = len(mos) == 2
            records["int"].append([int(index), int(bool(mos)), int(mixup), int("ud" in flips), int("lr" in flips), int(bool(luts)),
                                   labels_out.shape[0]] + cen + [top, left, nw, nh, len(warps)])
            records["tiles"].append(tiles); records["M"].append(Ms); records["s"].append(ss)
            records["r"].append(got.get("r", 0.0) if mixup else 0.0)
            records["gain"].append(got["g"] * [hyp["hsv_h"], hyp["hsv_s"], hyp["hsv_v"]] + 1 if "g" in got else np.ones(3))
            records["lut"].append(np.stack(luts) if luts else np.zeros((3, 256), np.uint8))
            records["labels"].append(labels_out.numpy())
    finally:
        DS.mosaic_augmentation, DA.get_transform_matrix = real_mosaic, real_tm
        np.random.beta, np.random.uniform, np.flipud, np.fliplr = real_beta, real_unif, real_ud, real_lr
    out = {name + "_" + k: np.stack(v) if k != "labels" else np.concatenate(v, 0).astype(np.float32) for k, v in records.items()}
    out[name + "_int"] = out[name + "_int"].astype(np.int64)
    out[name + "_sizes"] = np.array(sizes, np.int64)
    out[name + "_labels_in"] = np.concatenate(labels, 0)
    out[name + "_nlabels_in"] = np.array([len(l) for l in labels], np.int64)
    out[name + "_hyp"] = np.array(json.dumps(hyp))
    out[name + "_seed"] = np.array(seed, np.int64)
    ints = out[name + "_int"]
    print("%s: %d draws, %d mosaic, %d mixup, %d flipud, %d fliplr, %d labels" % (name, len(ints), ints[:, 1].sum(), ints[:, 2].sum(),
                                                                             ints[:, 3].sum(), ints[:, 4].sum(), ints[:, 6].sum()))
    return out


def main():
    DA, DS = load_reference()
    out = {}
    for k, (name, (hyp, max_labels)) in enumerate(SETS.items()):
        out.update(run_set(DA, DS, name, hyp, max_labels, 7 + k))
    path = os.path.join(ROOT, "tests", "golden", "augment_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s" % path)


if __name__ == "__main__":
    main()
