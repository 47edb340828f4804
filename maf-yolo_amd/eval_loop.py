"""The evaluation loop of the reference, `Evaler.predict_model` (yolov6/core/evaler.py:129-194) with its timing split (`speed_result`,
`eval_speed` :366-372), over the HIP path — the caller-side counterpart SURVEY.md 8(c) asks for:

    uint8 batch from the data loader -> (/255) -> model(imgs)[0] -> non_max_suppression(conf, iou, multi_label=True) -> COCO rows

    loop = EvalLoop(model, conf_thres=0.03, iou_thres=0.65, half=True, ids=coco_ids)
    pred_results = loop.predict_model(dataloader)        # list of {"image_id", "category_id", "bbox", "score"} (evaler.py:411-434)
    loop.eval_speed()                                    # {"pre-process": ms, "inference": ms, "NMS": ms} per image, like the reference logs

do_pr_metric=True adds the reference's in-process precision / recall / mAP (evaler.py:143-151, 182-238, 240-271; on by default in its
tools/eval.py) over metrics.PrMetric: each batch's NMS result and the loader's targets feed one HIP launch, and after the loop
`loop.pr_metric_result == (map50, map)` as on the reference's Evaler, `loop.pr_metric` holds the full result (p, r, f1, ap, ap_class, py,
nt, the confusion matrix when plot_confusion_matrix=True; drawing stays the caller's).  The returned COCO rows are the same either way.

do_coco_metric=True adds the pycocotools block of Evaler.eval_model (evaler.py:276-364) over cocoeval.CocoEval: `anno` is a CocoGt or the
path of the instances JSON; each batch's coco_rows output also feeds CocoEval.update (no host sync), and after the loop
`loop.coco_metric_result == (map50, map, map75, map_s, map_m, map_l)` as eval_model returns it ((0.0, 0.0) without any detection),
`loop.coco_eval` holds the CocoEval (eval, stats).  With is_coco the evaluated images are those of the batches seen (evaler.py:305-308).

Differences from the reference, all inside the same call sequence: `/255` is folded into the first kernel (uint8 images go to the engine as
they are: fold_preprocess=True; False converts like evaler.py:161-163), the NMS result stays on the device and the COCO rows of a batch are
one kernel + one device->host copy (post.py).  Everything else — data loader, plots — is the caller's, unchanged.
"""
import time
from pathlib import Path

import torch

from . import cocoeval as _cocoeval
from . import metrics as _metrics
from . import nms as _nms
from . import post as _post


def _time_sync(dev):
    torch.cuda.synchronize(dev)          # yolov6/utils/torch_utils.py:time_sync
    return time.time()


class EvalLoop:
    def __init__(self, model, conf_thres=0.03, iou_thres=0.65, half=True, ids=None, is_coco=True, scale_exact=False, fold_preprocess=True, device=None,
                 do_pr_metric=False, plot_confusion_matrix=False, do_coco_metric=False, anno=None):
        self.model = model.eval()
        if do_coco_metric and anno is None:
            raise _cocoeval.lib.MafError("EvalLoop(do_coco_metric=True) needs anno: a CocoGt or the instances JSON path")
        self.do_coco_metric, self.anno = do_coco_metric, anno
        self.coco_eval, self.coco_metric_result = None, None
        self.do_pr_metric, self.plot_confusion_matrix = do_pr_metric, plot_confusion_matrix
        self.pr_metric, self.pr_metric_result = None, None
        self.conf_thres, self.iou_thres, self.half = conf_thres, iou_thres, half           # tools/eval.py:29-30 defaults
        self.ids, self.is_coco, self.scale_exact = ids, is_coco, scale_exact
        self.fold_preprocess = fold_preprocess
        self.device = device if device is not None else next(model.parameters()).device
        self.speed_result = torch.zeros(4)                                                  # [images, pre-process s, inference s, NMS s] (evaler.py:36)
        if half:
            self.model.half()                                                               # evaler.py:112 (masters stay fp32: Model.half)
        else:
            self.model.float()

    def predict_model(self, dataloader):
        pred_results = []
        dev = self.device
        metric = _metrics.PrMetric(self.model.nc, confusion=self.plot_confusion_matrix) if self.do_pr_metric else None
        coco, seen_ids = None, []
        if self.do_coco_metric:
            gt = self.anno if isinstance(self.anno, _cocoeval.CocoGt) else _cocoeval.CocoGt(self.anno, device=dev)
            coco = _cocoeval.CocoEval(gt)
        for imgs, targets, paths, shapes in dataloader:
            # pre-process (evaler.py:160-164)
            t1 = _time_sync(dev)
            imgs = imgs.to(dev, non_blocking=True)
            if not (self.fold_preprocess and imgs.dtype == torch.uint8):
                imgs = imgs.half() if self.half else imgs.float()
                imgs /= 255
            self.speed_result[1] += _time_sync(dev) - t1
            # inference (:167-169); uint8 images: `/255` happens inside the first kernel
            t2 = _time_sync(dev)
            if imgs.dtype == torch.uint8:
                self.model.precision = "fp16" if self.half else "fp32"
            with torch.no_grad():
                outputs, _ = self.model(imgs)
            self.speed_result[2] += _time_sync(dev) - t2
            # post-process (:177-180): the detections stay on the device
            t3 = _time_sync(dev)
            raw = _nms.nms_raw(outputs, self.conf_thres, self.iou_thres, multi_label=True)
            self.speed_result[3] += _time_sync(dev) - t3
            self.speed_result[0] += imgs.shape[0]
            if metric is not None:                          # statistics per image (:195-238), queued behind the NMS: no host sync
                metric.update(raw[0], raw[2], targets.to(dev, non_blocking=True), imgs.shape[2:], shapes, self.scale_exact)
            # save result (:187)
            if coco is None:
                pred_results.extend(_post.convert_to_coco_format(raw, imgs, paths, shapes, self.ids, self.is_coco, self.scale_exact))
            else:                                           # the same rows also feed CocoEval, queued behind the NMS
                image_ids = [int(Path(p).stem) if self.is_coco else Path(p).stem for p in paths]
                seen_ids.extend(image_ids)
                packed, total = _post.coco_rows(raw[0], raw[2], shapes, self.ids, self.scale_exact)
                coco.update(packed, total, image_ids)
                pred_results.extend(_post.coco_results(packed, total, paths, self.is_coco))
        if metric is not None:                              # :240-268
            self.pr_metric = metric.compute()
            self.pr_metric_result = self.pr_metric.pr_metric_result
        if coco is not None:                                # eval_model's pycocotools block (:286-364)
            self.coco_eval = coco
            if not pred_results:
                self.coco_metric_result = (0.0, 0.0)
            else:
                if self.is_coco:
                    coco.params.imgIds = seen_ids
                coco.evaluate()
                coco.accumulate()
                s = coco.summarize()
                self.coco_metric_result = (s[1], s[0], s[2], s[3], s[4], s[5])
        return pred_results

    def eval_speed(self):
        n = max(1.0, self.speed_result[0].item())
        pre, inf, nms_t = (1000.0 * self.speed_result[1:] / n).tolist()
        return {"pre-process": pre, "inference": inf, "NMS": nms_t}
