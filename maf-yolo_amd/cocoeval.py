"""COCO bbox mAP on the device: the pycocotools block of Evaler.eval_model (yolov6/core/evaler.py:276-364) — COCO(anno), loadRes,
COCOeval(anno, pred, 'bbox'), evaluate(), accumulate(), summarize() — over csrc/cocoeval.hip.

    gt = CocoGt("instances_val2017.json")                  # parsed once, held on the device; reuse it every epoch
    ev = CocoEval(gt)
    for ...:                                                # per batch, no host synchronisation
        packed, total = coco_rows(rows, count, shapes, ids)
        ev.update(packed, total, image_ids)                 # or, from the reference's pred_results / predictions.json: ev.load_res(rows)
    ev.params.imgIds = seen_ids                              # optional, as eval_model narrows it for COCO
    ev.evaluate(); ev.accumulate(); ev.summarize()          # one device -> host copy, in accumulate()
    ev.stats[:6]                                             # mAP@.5:.95, mAP@.5, AP75, APs, APm, APl

The rules (tests/cocoeval_ref.py) are pycocotools 2.0's for iouType 'bbox' with useCats 1 and the default parameters: precision, recall and
scores equal its arrays bit for bit, -1 included.  Only params.imgIds and params.catIds may be narrowed.  Tensors must be on the HIP device:
CPU tensors raise MafError (there is no CPU path).
"""
import json
import os

import numpy as np
import torch

from . import lib

INT64_MAX = (1 << 63) - 1
_LUT_MAX = 1 << 20            # category ids that update() maps on the device: non-negative ints below this


def _default_params():
    return dict(iouThrs=np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True),
                recThrs=np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True),
                maxDets=[1, 10, 100], areaRng=[[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]],
                areaRngLbl=["all", "small", "medium", "large"])


def _pinned(arr, dev):
    return torch.from_numpy(np.ascontiguousarray(arr)).pin_memory().to(dev, non_blocking=True)


def _device(device):
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise lib.MafError("cocoeval runs on the HIP path only: got device %s%s (no CPU fallback)"
                           % (dev, "" if torch.cuda.is_available() else " and no HIP device"))
    return dev


class CocoGt:
    """The ground truth of an instances-format dict (or JSON file) on the device: per annotation, sorted by (image, category) cell with JSON
    order kept inside a cell, its bbox (fp64 xywh), area (the JSON field), crowd and nonzero-id flags, id; the sorted image and category
    ids and the cell offsets.  Annotations of images or categories the file does not list are dropped, as pycocotools' getAnnIds drops them."""

    def __init__(self, anno, device=None):
        if isinstance(anno, (str, os.PathLike)):
            with open(anno) as f:
                anno = json.load(f)
        self.device = _device(device)
        self.img_ids = sorted({im["id"] for im in anno.get("images", [])})
        self.cat_ids = sorted({c["id"] for c in anno.get("categories", [])})
        self.img_index = {v: i for i, v in enumerate(self.img_ids)}
        self.cat_index = {v: i for i, v in enumerate(self.cat_ids)}
        I, K = len(self.img_ids), len(self.cat_ids)
        if I == 0 or K == 0:
            raise lib.MafError("CocoGt needs at least one image and one category")
        cells, box, area, flags, ids = [], [], [], [], []
        seen = set()
        for a in anno.get("annotations", []):
            i, k = self.img_index.get(a["image_id"]), self.cat_index.get(a["category_id"])
            if a["id"] in seen:
                raise lib.MafError("CocoGt: annotation id %r appears twice" % (a["id"],))
            seen.add(a["id"])
            if i is None or k is None:
                continue
            cells.append(i * K + k)
            box.append([float(v) for v in a["bbox"]])
            area.append(float(a["area"]))
            flags.append((lib.COCO_GT_CROWD if a.get("iscrowd", 0) else 0) | (lib.COCO_GT_IDNZ if a["id"] else 0))
            ids.append(a["id"])
        cells = np.asarray(cells, np.int64)
        perm = np.argsort(cells, kind="stable")
        counts = np.bincount(cells, minlength=I * K) if len(cells) else np.zeros(I * K, np.int64)
        if len(cells) and counts.max() > lib.COCO_MAX_GT:
            c = int(counts.argmax())
            raise lib.MafError("CocoGt: image %r holds %d annotations of category %r; at most %d per (image, category) are supported"
                               % (self.img_ids[c // K], int(counts.max()), self.cat_ids[c % K], lib.COCO_MAX_GT))
        off = np.zeros(I * K + 1, np.int64)
        np.cumsum(counts, out=off[1:])
        n = max(1, len(cells))                                # device buffers are never empty
        dev = self.device
        self.n_ann = len(cells)
        self.ann_ids = [ids[j] for j in perm]
        self.box = torch.zeros(n, 4, dtype=torch.float64, device=dev)
        self.area = torch.zeros(n, dtype=torch.float64, device=dev)
        self.flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        if len(cells):
            self.box.copy_(torch.from_numpy(np.asarray(box, np.float64)[perm]))
            self.area.copy_(torch.from_numpy(np.asarray(area, np.float64)[perm]))
            self.flags.copy_(torch.from_numpy(np.asarray(flags, np.uint8)[perm]))
        self.img = torch.from_numpy((cells[perm] // K).astype(np.int32)).to(dev)
        self.cat = torch.from_numpy((cells[perm] % K).astype(np.int32)).to(dev)
        self.off = torch.from_numpy(off).to(dev)
        ints = all(isinstance(c, int) and not isinstance(c, bool) and 0 <= c < _LUT_MAX for c in self.cat_ids)
        self.cat_lut = None
        if ints:
            lut = np.full(self.cat_ids[-1] + 1, -1, np.int32)
            lut[self.cat_ids] = np.arange(K, dtype=np.int32)
            self.cat_lut = torch.from_numpy(lut).to(dev)

    @property
    def num_images(self):
        return len(self.img_ids)

    @property
    def num_categories(self):
        return len(self.cat_ids)


class Params:
    """COCOeval.params for iouType 'bbox' (pycocotools' setDetParams)."""

    def __init__(self, gt):
        self.imgIds = list(gt.img_ids)
        self.catIds = list(gt.cat_ids)
        for k, v in _default_params().items():
            setattr(self, k, v)
        self.iouType = "bbox"
        self.useCats = 1


class CocoEval:
    """The part of COCOeval(anno, pred, 'bbox') that Evaler.eval_model uses.  eval = {"params", "counts", "precision" [T, R, K, A, M],
    "recall" [T, K, A, M], "scores" [T, R, K, A, M]} as NumPy arrays after accumulate(); stats [12] after summarize()."""

    def __init__(self, gt, img_ids=None):
        if not isinstance(gt, CocoGt):
            raise lib.MafError("CocoEval takes a CocoGt")
        self.gt = gt
        self.params = Params(gt)
        if img_ids is not None:
            self.params.imgIds = list(img_ids)
        self.eval, self.stats = {}, []
        self._chunks = []                                     # per update / load_res: (img, cat, box, score) device tensors
        self._keep = []
        self._ev = None

    # ---- results
    def update(self, packed, total, image_ids, stream=None):
        """One batch of post.coco_rows: packed [R, 7] fp32 (batch image, category id, x, y, w, h, score), total [1] int32, image_ids: the
        batch's image ids (the `image_id` of its rows).  One host -> device copy, no host synchronisation."""
        for t in (packed, total):
            if not (torch.is_tensor(t) and t.is_cuda):
                raise lib.MafError("CocoEval.update runs on the HIP path only: got a %s (no CPU fallback)" %
                                   (t.device if torch.is_tensor(t) else type(t).__name__))
        if self.gt.cat_lut is None:
            raise lib.MafError("CocoEval.update maps category ids on the device: they must be ints in [0, %d); use load_res" % _LUT_MAX)
        if packed.dtype != torch.float32 or packed.dim() != 2 or packed.shape[1] != 7 or total.dtype != torch.int32:
            raise lib.MafError("CocoEval.update takes coco_rows' packed fp32 [R, 7] and total int32 [1]")
        idx = np.empty(len(image_ids), np.int32)
        for b, v in enumerate(image_ids):
            i = self.gt.img_index.get(v)
            if i is None:
                raise lib.MafError("CocoEval: result image id %r is not an image of the ground truth" % (v,))
            idx[b] = i
        rows = int(packed.shape[0])
        if rows == 0 or len(idx) == 0:
            return
        dev = self.gt.device
        idx_t = _pinned(idx, dev)                            # the one host -> device copy
        packed = packed.contiguous()
        img = torch.empty(rows, dtype=torch.int32, device=dev)
        cat = torch.empty(rows, dtype=torch.int32, device=dev)
        box = torch.empty(rows, 4, dtype=torch.float64, device=dev)
        score = torch.empty(rows, dtype=torch.float64, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        lib.check(lib.load().maf_coco_append(packed.data_ptr(), total.data_ptr(), rows, idx_t.data_ptr(), len(idx), self.gt.cat_lut.data_ptr(),
                                             self.gt.cat_lut.numel(), img.data_ptr(), cat.data_ptr(), box.data_ptr(), score.data_ptr(),
                                             st.cuda_stream))
        self._keep.append((packed, total, idx_t))            # alive until evaluate() has queued behind them
        self._chunks.append((img, cat, box, score))

    def load_res(self, results):
        """The reference's pred_results (a list of {"image_id", "category_id", "bbox", "score"}) or a predictions.json path, as
        COCO.loadRes reads them: image ids must be gt images; categories outside the gt's are dropped at evaluate()."""
        if isinstance(results, (str, os.PathLike)):
            with open(results) as f:
                results = json.load(f)
        n = len(results)
        if n == 0:
            return
        img = np.empty(n, np.int32)
        cat = np.empty(n, np.int32)
        box = np.empty((n, 4), np.float64)
        score = np.empty(n, np.float64)
        for j, r in enumerate(results):
            i = self.gt.img_index.get(r["image_id"])
            if i is None:
                raise lib.MafError("CocoEval: result image id %r is not an image of the ground truth" % (r["image_id"],))
            img[j] = i
            cat[j] = self.gt.cat_index.get(r["category_id"], -1)
            box[j] = r["bbox"]
            score[j] = r["score"]
        dev = self.gt.device
        self._chunks.append(tuple(torch.from_numpy(a).to(dev) for a in (img, cat, box, score)))

    # ---- evaluation
    def _check_params(self):
        p, d = self.params, _default_params()
        if p.iouType != "bbox" or p.useCats != 1:
            raise lib.MafError("CocoEval covers iouType 'bbox' with useCats 1 only")
        for k, v in d.items():
            if not np.array_equal(np.asarray(getattr(p, k), dtype=object if k == "areaRngLbl" else np.float64),
                                  np.asarray(v, dtype=object if k == "areaRngLbl" else np.float64)):
                raise lib.MafError("CocoEval: params.%s must keep its bbox default (only imgIds and catIds may be narrowed)" % k)
        p.imgIds = list(np.unique(p.imgIds))                  # as COCOeval.evaluate
        p.catIds = list(np.unique(p.catIds))

    def evaluate(self):
        """evaluateImg over every (image, category) cell: the match records on the device (no host sync)."""
        self._check_params()
        gt, p, dev = self.gt, self.params, self.gt.device
        I, K = gt.num_images, gt.num_categories
        sel = np.zeros(I, np.uint8)
        for v in p.imgIds:
            i = gt.img_index.get(v.item() if isinstance(v, np.generic) else v)
            if i is not None:
                sel[i] = 1
        cat_of = np.array([gt.cat_index.get(v.item() if isinstance(v, np.generic) else v, -1) for v in p.catIds], np.int32)
        cat_map = np.full(K, -1, np.int32)
        for kp, k in enumerate(cat_of):
            if k >= 0:
                cat_map[k] = kp
        if self._chunks:
            img, cat, box, score = (torch.cat([c[j] for c in self._chunks]) for j in range(4))
        else:
            img = cat = torch.full((1,), -1, dtype=torch.int32, device=dev)
            box, score = torch.zeros(1, 4, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
        n = img.numel()
        img_sel, cat_map_t = _pinned(sel, dev), _pinned(cat_map, dev)
        # stable order by (cell, score descending): results-list order breaks ties, as pycocotools' mergesort of -score in a cell
        _, p1 = torch.sort(-score, stable=True)
        i1, c1 = img[p1].long(), cat[p1].long()
        ok = (i1 >= 0) & (c1 >= 0)
        ok &= img_sel[i1.clamp(min=0)].bool() & (cat_map_t[c1.clamp(min=0)] >= 0)
        keys = torch.where(ok, i1 * K + c1, torch.full_like(i1, INT64_MAX))
        cell_keys, p2 = torch.sort(keys, stable=True)
        order = p1[p2].contiguous()
        rank = torch.full((n,), -1, dtype=torch.int32, device=dev)
        mbits = torch.zeros(n, dtype=torch.int64, device=dev)
        ibits = torch.zeros(n, dtype=torch.int64, device=dev)
        npig = torch.empty(I * K * lib.COCO_A, dtype=torch.int32, device=dev)
        d = _default_params()
        iou_thrs, area_rng = _pinned(np.asarray(d["iouThrs"], np.float64), dev), _pinned(np.asarray(d["areaRng"], np.float64).reshape(-1), dev)
        lib.check(lib.load().maf_coco_match(gt.box.data_ptr(), gt.area.data_ptr(), gt.flags.data_ptr(), gt.off.data_ptr(), cell_keys.data_ptr(),
                                            order.data_ptr(), box.data_ptr(), n, img_sel.data_ptr(), cat_map_t.data_ptr(), I, K,
                                            iou_thrs.data_ptr(), area_rng.data_ptr(), rank.data_ptr(), mbits.data_ptr(), ibits.data_ptr(),
                                            npig.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        self._ev = dict(n=n, order=order, score=score[order], cat=cat[order], rank=rank, mbits=mbits, ibits=ibits, npig=npig, img_sel=img_sel,
                        cat_map=cat_map_t, cat_of=_pinned(cat_of, dev), Kp=len(cat_of),
                        keep=(iou_thrs, area_rng, box, cell_keys))
        self._keep = []

    def accumulate(self):
        """precision / recall / scores on the device, then ONE device -> host copy."""
        if self._ev is None:
            raise lib.MafError("CocoEval.accumulate: run evaluate() first")
        e, gt, dev = self._ev, self.gt, self.gt.device
        I, K, Kp, n = gt.num_images, gt.num_categories, e["Kp"], e["n"]
        T, R, A, M = lib.COCO_T, lib.COCO_R, lib.COCO_A, lib.COCO_M
        # stable order of the kept detections by (category, score descending); ties keep image order, then rank in the cell
        _, p3 = torch.sort(-e["score"], stable=True)
        kept = e["rank"] >= 0
        ck = torch.where(kept, e["cat_map"][e["cat"].long().clamp(min=0)].long(), torch.full((n,), INT64_MAX, dtype=torch.int64, device=dev))
        cat_keys, p4 = torch.sort(ck[p3], stable=True)
        pos = p3[p4]
        rank, mbits, ibits, score = (e[k][pos].contiguous() for k in ("rank", "mbits", "ibits", "score"))
        d = _default_params()
        rec_thrs = _pinned(np.asarray(d["recThrs"], np.float64), dev)
        max_dets = _pinned(np.asarray(d["maxDets"], np.int32), dev)
        np_ = T * R * Kp * A * M
        out = torch.empty(2 * np_ + T * Kp * A * M, dtype=torch.float64, device=dev)
        lib.check(lib.load().maf_coco_accumulate(cat_keys.data_ptr(), rank.data_ptr(), mbits.data_ptr(), ibits.data_ptr(), score.data_ptr(), n,
                                                 e["npig"].data_ptr(), e["img_sel"].data_ptr(), e["cat_of"].data_ptr(), I, K, Kp,
                                                 rec_thrs.data_ptr(), max_dets.data_ptr(), out.data_ptr(), out.data_ptr() + 8 * 2 * np_,
                                                 out.data_ptr() + 8 * np_, torch.cuda.current_stream(dev).cuda_stream))
        h = out.cpu().numpy()                                 # the one host sync
        self.eval = {"params": self.params, "counts": [T, R, Kp, A, M],
                     "precision": h[:np_].reshape(T, R, Kp, A, M), "scores": h[np_:2 * np_].reshape(T, R, Kp, A, M),
                     "recall": h[2 * np_:].reshape(T, Kp, A, M)}

    def summarize(self):
        """pycocotools' _summarizeDets on the host over eval: prints its 12 lines, sets stats."""
        if not self.eval:
            raise Exception("Please run accumulate() first")
        self.stats = summarize(self.eval, self.params)
        return self.stats


def _summarize_one(ev, p, ap=1, iouThr=None, areaRng="all", maxDets=100):
    iStr = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}"
    titleStr = "Average Precision" if ap == 1 else "Average Recall"
    typeStr = "(AP)" if ap == 1 else "(AR)"
    iouStr = "{:0.2f}:{:0.2f}".format(p.iouThrs[0], p.iouThrs[-1]) if iouThr is None else "{:0.2f}".format(iouThr)
    aind = [i for i, aRng in enumerate(p.areaRngLbl) if aRng == areaRng]
    mind = [i for i, mDet in enumerate(p.maxDets) if mDet == maxDets]
    if ap == 1:
        s = ev["precision"]
        if iouThr is not None:
            t = np.where(iouThr == p.iouThrs)[0]
            s = s[t]
        s = s[:, :, :, aind, mind]
    else:
        s = ev["recall"]
        if iouThr is not None:
            t = np.where(iouThr == p.iouThrs)[0]
            s = s[t]
        s = s[:, :, aind, mind]
    if len(s[s > -1]) == 0:
        mean_s = -1
    else:
        mean_s = np.mean(s[s > -1])
    print(iStr.format(titleStr, typeStr, iouStr, areaRng, maxDets, mean_s))
    return mean_s


def summarize(ev, p):
    """_summarizeDets: stats [12] from eval's precision / recall (host NumPy, as pycocotools)."""
    stats = np.zeros((12,))
    stats[0] = _summarize_one(ev, p, 1)
    stats[1] = _summarize_one(ev, p, 1, iouThr=.5, maxDets=p.maxDets[2])
    stats[2] = _summarize_one(ev, p, 1, iouThr=.75, maxDets=p.maxDets[2])
    stats[3] = _summarize_one(ev, p, 1, areaRng="small", maxDets=p.maxDets[2])
    stats[4] = _summarize_one(ev, p, 1, areaRng="medium", maxDets=p.maxDets[2])
    stats[5] = _summarize_one(ev, p, 1, areaRng="large", maxDets=p.maxDets[2])
    stats[6] = _summarize_one(ev, p, 0, maxDets=p.maxDets[0])
    stats[7] = _summarize_one(ev, p, 0, maxDets=p.maxDets[1])
    stats[8] = _summarize_one(ev, p, 0, maxDets=p.maxDets[2])
    stats[9] = _summarize_one(ev, p, 0, areaRng="small", maxDets=p.maxDets[2])
    stats[10] = _summarize_one(ev, p, 0, areaRng="medium", maxDets=p.maxDets[2])
    stats[11] = _summarize_one(ev, p, 0, areaRng="large", maxDets=p.maxDets[2])
    return stats
