"""Golden vectors for copy_paste and mask_refine on polygon labels (maf-yolo_amd/augment.py TrainAugment(polygons=True)): the reference's OWN
TrainValDataset.__getitem__ (yolov6/data/datasets.py:147-275 with mosaic_augmentation, copy_paste, random_affine(mask_refine=True),
resample_segments, segment2box) run on the stand-in dataset of tools/make_golden_augment.py, with seeded polygon labels.

    python tools/make_golden_copy_paste.py        ->  tests/golden/copy_paste_cases.npz

cv2 is stubbed as in make_golden_augment.py; drawContours and flip are stubbed too and record their arguments (flip returns the mirrored
array, drawContours draws nothing).  Recorded per sample: what the augment fixture records, the int32 contours handed to drawContours per
layer (layer 0: the sample's mosaic, layer 1: the cached mosaic), labels_out, how often segment2box took its np.zeros((1, 4)) fallback and how
many pasted objects box_candidates dropped; per set, the value of random.random() drawn right after the last sample.  Three hyp sets: the
MAF-YOLO-n defaults, MAF-YOLO-m's (copy_paste 0.2, mixup 0.1, dy_mixup 0.4) and a stress set (copy_paste 1.0, degrees 5, shear 2 on m's).
Data only: nothing of the reference is stored."""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_augment as G  # noqa: E402

HYP_M = dict(G.HYP_N, copy_paste=0.2, mixup=0.1, dy_mixup=0.4)
SETS = {
    "n": G.HYP_N,
    "m": HYP_M,
    "stress": dict(HYP_M, copy_paste=1.0, degrees=5.0, shear=2.0),
}
DRAWS = 100
MAX_LABELS = 5


def polygon_labels(rs, n_img, max_labels):
    """Per image: float32 polygons (3..12 vertices around a seeded centre, normalised, inside [0, 1]) and the [n, 5] box labels the
    reference's label reader derives from them (segments2boxes: min / max -> xywh)."""
    segments, labels = [], []
    for _ in range(n_img):
        n = int(rs.randint(0, max_labels + 1))
        segs, rows = [], []
        for _ in range(n):
            k = int(rs.randint(3, 13))
            c = rs.uniform(0.1, 0.9, 2)
            rad = rs.uniform(0.02, 0.3, 2)
            ang = np.sort(rs.uniform(0, 2 * np.pi, k))
            jit = rs.uniform(0.5, 1.0, k)
            xy = np.stack([c[0] + rad[0] * jit * np.cos(ang), c[1] + rad[1] * jit * np.sin(ang)], 1).clip(0, 1).astype(np.float32)
            segs.append(xy)
            x0, y0, x1, y1 = xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max()
            rows.append([float(rs.randint(0, 80)), (x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0])
        segments.append(segs)
        labels.append(np.array(rows, np.float32).reshape(-1, 5))
    return segments, labels


def run_set(DA, DS, name, hyp, seed):
    rs = np.random.RandomState(seed)
    sizes, _ = G.dataset(rs, 40, 0)
    segments, labels = polygon_labels(rs, len(sizes), MAX_LABELS)
    self = object.__new__(DS.TrainValDataset)
    self.__dict__.update(augment=True, hyp=dict(hyp), img_size=640, rect=False, albument=False, dy_cache_mixup=True,
                         img_paths=["%d_%d_%d.jpg" % (i, h, w) for i, (h, w) in enumerate(sizes)], labels=labels,
                         segments=[s if s else np.zeros((0, 5), np.float32) for s in segments], all_results_cache=[],
                         max_cached_images=20, random_pop=False, num=0, num1=0, small_num=0)
    order = rs.randint(0, len(sizes), DRAWS)
    records = dict(int=[], tiles=[], M=[], s=[], r=[], gain=[], lut=[], labels=[], ncontours=[], extra=[])
    contours = []
    mos, tm, drawn, stat = [], [], [], dict(fallback=0, dropped=0, pasted=[])
    real = dict(mosaic=DS.mosaic_augmentation, tm=DA.get_transform_matrix, cp=DA.copy_paste, s2b=DA.segment2box, bc=DA.box_candidates)
    cv2 = sys.modules["cv2"]

    def mosaic(img_size, imgs, hs, ws, labels, hyp, segments=None):
        state = DA.random.getstate()
        yc, xc = (int(DA.random.uniform(img_size // 2, 3 * img_size // 2)) for _ in range(2))
        DA.random.setstate(state)
        mos.append(([G._tag(im) for im in imgs], list(zip(hs, ws)), (xc, yc)))
        return real["mosaic"](img_size, imgs, hs, ws, labels, hyp, segments)

    def transform(*a, **k):
        M, s = real["tm"](*a, **k)
        tm.append((np.array(M), s))
        return M, s

    def copy_paste(im, labels, segments, p=0.5):
        n0 = len(labels)
        out = real["cp"](im, labels, segments, p=p)
        stat["pasted"].append((n0, len(out[1])))
        return out

    def segment2box(*a, **k):
        box = real["s2b"](*a, **k)
        stat["fallback"] += int(np.ndim(box) == 2)
        return box

    def box_candidates(*a, **k):
        keep = real["bc"](*a, **k)
        if stat["pasted"] and len(keep) == stat["pasted"][-1][1]:          # the random_affine of the mosaic copy_paste just extended
            stat["dropped"] += int((~keep[stat["pasted"][-1][0]:]).sum())
        return keep

    def draw_contours(img, cnts, idx, color, thickness):
        assert idx == -1 and thickness == cv2.FILLED and len(cnts) == 1 and cnts[0].dtype == np.int32
        drawn.append((len(mos) - 1, np.array(cnts[0])))
        return img

    cv2.__dict__.update(drawContours=draw_contours, flip=lambda im, code: np.ascontiguousarray(im[:, ::-1]), FILLED=-1)
    real_beta, real_unif = np.random.beta, np.random.uniform
    got = {}
    np.random.beta = lambda *a: got.setdefault("r", real_beta(*a))
    np.random.uniform = lambda *a: got.setdefault("g", real_unif(*a))
    flips = []
    real_ud, real_lr = np.flipud, np.fliplr
    np.flipud = lambda m: (flips.append("ud"), real_ud(m))[1]
    np.fliplr = lambda m: (flips.append("lr"), real_lr(m))[1]
    DS.mosaic_augmentation, DA.get_transform_matrix, DA.copy_paste, DA.segment2box, DA.box_candidates = (mosaic, transform, copy_paste,
                                                                                                          segment2box, box_candidates)
    random.seed(seed)
    np.random.seed(seed)
    try:
        for index in order:
            G.LOG.clear(); mos.clear(); tm.clear(); flips.clear(); got.clear(); drawn.clear()
            stat.update(fallback=0, dropped=0, pasted=[])
            img, labels_out, _, _ = DS.TrainValDataset.__getitem__(self, int(index))
            assert tuple(img.shape) == (3, 640, 640) and mos, "every draw of these sets is a mosaic"
            luts = [e[1] for e in G.LOG if e[0] == "lut"]
            tiles = np.full((8, 3), -1, np.int64)
            cen = [-1] * 4
            for k, (idx, hw, c) in enumerate(mos):
                tiles[4 * k:4 * k + 4, 0] = idx
                tiles[4 * k:4 * k + 4, 1:] = hw
                cen[2 * k:2 * k + 2] = c
            Ms = np.zeros((2, 3, 3)); ss = np.zeros(2)
            for k, (M, s) in enumerate(tm):
                Ms[k], ss[k] = M, s
            mixup = len(mos) == 2
            records["int"].append([int(index), 1, int(mixup), int("ud" in flips), int("lr" in flips), int(bool(luts)), labels_out.shape[0]] + cen)
            records["tiles"].append(tiles); records["M"].append(Ms); records["s"].append(ss)
            records["r"].append(got.get("r", 0.0) if mixup else 0.0)
            records["gain"].append(got["g"] * [hyp["hsv_h"], hyp["hsv_s"], hyp["hsv_v"]] + 1 if "g" in got else np.ones(3))
            records["lut"].append(np.stack(luts) if luts else np.zeros((3, 256), np.uint8))
            records["labels"].append(labels_out.numpy())
            records["ncontours"].append([sum(1 for l, _ in drawn if l == k) for k in range(2)])
            records["extra"].append([stat["fallback"], stat["dropped"]])
            assert [l for l, _ in drawn] == sorted(l for l, _ in drawn)
            contours.extend(c for _, c in drawn)
        after = random.random()
    finally:
        DS.mosaic_augmentation, DA.get_transform_matrix, DA.copy_paste, DA.segment2box, DA.box_candidates = (real[k] for k in
                                                                                                              ("mosaic", "tm", "cp", "s2b", "bc"))
        np.random.beta, np.random.uniform, np.flipud, np.fliplr = real_beta, real_unif, real_ud, real_lr
    out = {name + "_" + k: np.stack(v) if k != "labels" else np.concatenate(v, 0).astype(np.float32) for k, v in records.items()}
    for k in ("int", "ncontours", "extra"):
        out[name + "_" + k] = out[name + "_" + k].astype(np.int64)
    out[name + "_lut"] = out[name + "_lut"].astype(np.uint8)
    out[name + "_contour_xy"] = np.concatenate(contours + [np.zeros((0, 2), np.int32)], 0).astype(np.int32)
    out[name + "_contour_len"] = np.array([len(c) for c in contours], np.int64)
    out[name + "_sizes"] = np.array(sizes, np.int64)
    out[name + "_labels_in"] = np.concatenate(labels, 0)
    out[name + "_nlabels_in"] = np.array([len(l) for l in labels], np.int64)
    out[name + "_seg_xy"] = np.concatenate([s for segs in segments for s in segs], 0).astype(np.float32)
    out[name + "_seg_len"] = np.array([len(s) for segs in segments for s in segs], np.int64)
    out[name + "_after"] = np.array(after, np.float64)
    out[name + "_hyp"] = np.array(json.dumps(hyp))
    out[name + "_seed"] = np.array(seed, np.int64)
    ints, nc, ex = out[name + "_int"], out[name + "_ncontours"], out[name + "_extra"]
    print("%s: %d draws, %d mixup, pasted %d + %d contours (%d / %d samples), %d fallbacks, %d pasted dropped, %d labels" %
          (name, len(ints), ints[:, 2].sum(), nc[:, 0].sum(), nc[:, 1].sum(), (nc[:, 0] > 0).sum(), (nc[:, 1] > 0).sum(), ex[:, 0].sum(),
           ex[:, 1].sum(), ints[:, 6].sum()))
    return out


def main():
    DA, DS = G.load_reference()
    out = {}
    for k, (name, hyp) in enumerate(SETS.items()):
        out.update(run_set(DA, DS, name, hyp, 11 + k))
    path = os.path.join(ROOT, "tests", "golden", "copy_paste_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
