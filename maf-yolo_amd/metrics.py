"""Precision, recall and mAP of an evaluation on the device: the `do_pr_metric` path of Evaler.predict_model (yolov6/core/evaler.py:143-151,
182-238, 240-271) with yolov6/utils/metrics.py process_batch, ConfusionMatrix, ap_per_class and compute_ap, over csrc/pr_metric.hip.

    metric = PrMetric(nc=80, confusion=True)
    for ...:                                                          # per batch, no host synchronisation
        rows, idx, count = nms_raw(pred, 0.03, 0.65, multi_label=True)
        metric.update(rows, count, targets, imgs.shape[2:], shapes)  # targets: the loader's [N, 6] on the device
    res = metric.compute()                                            # one device -> host copy
    res.map50, res.map, res.p, res.r, res.ap, res.f1, res.ap_class, res.matrix

The rules (tests/pr_metric_ref.py) are the reference's, with two orderings it leaves to NumPy's unstable sort fixed: equal IoUs go to the lower
label index (and, in the confusion matrix, to the lower detection index); equal confidences keep image order, then NMS row order.  Tensors
must be on the HIP device: CPU tensors raise MafError (there is no CPU path).
"""
import numpy as np
import torch

from . import lib

INT64_MAX = (1 << 63) - 1


def default_iouv():
    return torch.linspace(0.5, 0.95, 10)                       # evaler.py:146


def _on_device(*ts):
    for t in ts:
        if torch.is_tensor(t) and not t.is_cuda:
            raise lib.MafError("metrics run on the HIP path only: got a %s tensor (no CPU fallback)" % t.device)


def _check(rc):
    lib.check(rc)


def _pinned(arr, dev):
    return torch.from_numpy(np.ascontiguousarray(arr)).pin_memory().to(dev, non_blocking=True)


def _iouv_dev(iouv, dev):
    iouv = default_iouv() if iouv is None else iouv
    if torch.is_tensor(iouv) and iouv.is_cuda:
        return iouv.float().contiguous()
    return _pinned(np.asarray(iouv.cpu() if torch.is_tensor(iouv) else iouv, np.float32), dev)


def _error_text(bits):
    why = []
    if bits & lib.PR_ERR_CLASS:
        why.append("a class outside [0, nc) or not integral")
    if bits & lib.PR_ERR_LABELS:
        why.append("an image with more than %d labels" % lib.PR_MAX_LABELS)
    if bits & lib.PR_ERR_CAPACITY:
        why.append("records past the buffer")
    return ", ".join(why)


def _curves(keys, masks, state, nc, niou, stream=None):
    """Stable sort of the keys (device), then maf_pr_curves -> fp64 output tensor on the device."""
    n = keys.numel()
    skeys, perm = torch.sort(keys, stable=True)
    L = lib.load()
    wsb = L.maf_pr_workspace_bytes(nc, niou, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=keys.device)
    out = torch.empty(L.maf_pr_out_doubles(nc, niou), dtype=torch.float64, device=keys.device)
    st = stream if stream is not None else torch.cuda.current_stream(keys.device)
    _check(L.maf_pr_curves(skeys.data_ptr(), perm.data_ptr(), masks.data_ptr(), n, state.data_ptr(), nc, niou, ws.data_ptr(), wsb,
                           out.data_ptr(), st.cuda_stream))
    return out


def _split(h, nc, niou):
    o = lib.PR_HEADER
    parts = {}
    for name in ("p", "r", "f1", "py"):
        parts[name] = h[o:o + nc * 1000].reshape(nc, 1000)
        o += nc * 1000
    parts["ap"] = h[o:o + nc * niou].reshape(nc, niou)
    o += nc * niou
    parts["nt"] = h[o:o + nc].astype(np.int64)
    o += nc
    parts["matrix"] = h[o:o + (nc + 1) ** 2].reshape(nc + 1, nc + 1).copy()
    return parts


class PrMetricResult:
    """What Evaler.predict_model derives (evaler.py:240-268).  p, r, f1, py [nc_present, 1000], ap [nc_present, niou], ap_class: the rows of
    the classes that have labels (np.unique of the target classes); py rows of classes without predictions are 0.  When no row is correct at
    any threshold, map50 = map = 0.0 and the curves are None, as the reference logs "Calculate metric failed"."""

    def __init__(self, seen, nt, matrix, ok, p=None, r=None, ap=None, f1=None, ap_class=None, py=None, f1_index=None,
                 mp=0.0, mr=0.0, mf1=0.0, map50=0.0, map=0.0):
        self.seen, self.nt, self.matrix, self.ok = seen, nt, matrix, ok
        self.p, self.r, self.ap, self.f1, self.ap_class, self.py, self.f1_index = p, r, ap, f1, ap_class, py, f1_index
        self.mp, self.mr, self.mf1, self.map50, self.map = mp, mr, mf1, map50, map

    @property
    def pr_metric_result(self):
        return (self.map50, self.map)

    def __repr__(self):
        return "PrMetricResult(seen=%d, labels=%d, mp=%.4g, mr=%.4g, map50=%.4g, map=%.4g)" % (self.seen, int(self.nt.sum()), self.mp, self.mr,
                                                                                           self.map50, self.map)


class PrMetric:
    """The statistics block of Evaler.predict_model: update() per batch with the NMS result before any rescale, compute() once."""

    def __init__(self, nc, iouv=None, confusion=False, conf=0.25, iou_thres=0.45):
        if not 0 < nc <= lib.PR_MAX_CLASSES:
            raise lib.MafError("PrMetric supports 1..%d classes, got %d" % (lib.PR_MAX_CLASSES, nc))
        self.nc, self.iouv, self.confusion, self.cm_conf, self.cm_iou = int(nc), iouv, bool(confusion), float(conf), float(iou_thres)
        self.niou = len(default_iouv() if iouv is None else iouv)
        if not 0 < self.niou <= 16:
            raise lib.MafError("PrMetric takes 1..16 IoU thresholds, got %d" % self.niou)
        self.reset()

    def reset(self):
        self.seen, self.bound, self.batches = 0, 0, 0
        self.dev = self.state = self.offs = self.keys = self.masks = self._iouv = None

    def _grow(self, need):
        cap = self.keys.numel() if self.keys is not None else 0
        if need > cap:
            new = max(need, 2 * cap, 4096)
            keys = torch.full((new,), INT64_MAX, dtype=torch.int64, device=self.dev)
            masks = torch.zeros(new, dtype=torch.int16, device=self.dev)
            if cap:
                keys[:cap].copy_(self.keys)
                masks[:cap].copy_(self.masks)
            self.keys, self.masks = keys, masks
        if self.batches + 2 > self.offs.numel():
            offs = torch.zeros(2 * self.offs.numel(), dtype=torch.int64, device=self.dev)
            offs[:self.offs.numel()].copy_(self.offs)
            self.offs = offs

    def update(self, rows, count, targets, img_hw, shapes, scale_exact=False, stream=None):
        """rows [B, max_det, 6] fp32, count [B] int32 (nms_raw), targets [N, 6] fp32 (image, class, x, y, w, h normalised to the
        letterboxed img_hw = (H, W)), shapes: the loader's ((h0, w0), ((gain_h, gain_w), (pad_w, pad_h))) per image.  No host sync."""
        _on_device(rows, count, targets)
        B, max_det = int(rows.shape[0]), int(rows.shape[1])
        if max_det > lib.PR_MAX_DET:
            raise lib.MafError("PrMetric supports max_det <= %d, got %d" % (lib.PR_MAX_DET, max_det))
        if self.dev is None:
            self.dev = rows.device
            L = lib.load()
            self.state = torch.zeros(L.maf_pr_state_ints(self.nc), dtype=torch.int32, device=self.dev)
            self.offs = torch.zeros(64, dtype=torch.int64, device=self.dev)
            self._iouv = _iouv_dev(self.iouv, self.dev)
        self._grow(self.bound + B * max_det)
        par = np.empty((B, 6), np.float32)
        for i, s in enumerate(shapes):
            (h0, w0), (gain, pad) = s[0], s[1]
            par[i] = (h0, w0, gain[1] if scale_exact else gain[0], gain[0], pad[0], pad[1])
        par_t = _pinned(par, self.dev)
        rows = rows if rows.dtype == torch.float32 and rows.is_contiguous() else rows.float().contiguous()
        count = count if count.dtype == torch.int32 else count.int()
        targets = targets.float().contiguous().reshape(-1, 6)
        H, W = int(img_hw[0]), int(img_hw[1])
        st = stream if stream is not None else torch.cuda.current_stream(self.dev)
        flags = lib.PR_CONFUSION if self.confusion else 0
        o = self.offs.data_ptr() + 8 * self.batches
        _check(lib.load().maf_pr_match(rows.data_ptr(), count.data_ptr(), B, max_det, targets.data_ptr() if targets.numel() else None,
                                       targets.shape[0], par_t.data_ptr(), H, W, self._iouv.data_ptr(), self.niou, self.nc, flags,
                                       self.cm_conf, self.cm_iou, o, o + 8, self.keys.data_ptr(), self.masks.data_ptr(), self.keys.numel(),
                                       self.state.data_ptr(), st.cuda_stream))
        self._keep = (rows, count, targets, par_t)            # alive until the next update / compute has been queued behind them
        self.seen += B
        self.bound += B * max_det
        self.batches += 1

    def compute(self):
        """-> PrMetricResult, after ONE device -> host copy.  Raises MafError for the device-side errors of any batch."""
        nc, niou = self.nc, self.niou
        if self.dev is None:
            return PrMetricResult(0, np.zeros(nc, np.int64), np.zeros((nc + 1, nc + 1)) if self.confusion else None, False)
        out = _curves(self.keys[:self.bound], self.masks[:self.bound], self.state, nc, niou)
        h = out.cpu().numpy()                                 # the one host sync
        self._keep = None
        bits = int(h[8])
        if bits:
            raise lib.MafError("PrMetric: %s" % _error_text(bits))
        parts = _split(h, nc, niou)
        matrix = parts["matrix"] if self.confusion else None
        if not h[7]:
            return PrMetricResult(self.seen, parts["nt"], matrix, False)
        present = parts["nt"] > 0
        return PrMetricResult(self.seen, parts["nt"], matrix, True, p=parts["p"][present], r=parts["r"][present], ap=parts["ap"][present],
                              f1=parts["f1"][present], ap_class=np.nonzero(present)[0].astype(np.int32), py=parts["py"][present],
                              f1_index=int(h[0]), mp=float(h[1]), mr=float(h[2]), mf1=float(h[3]), map50=float(h[4]), map=float(h[5]))


def _match_one(detections, labels, iouv, nc, flags, state, cm_conf=0.25, cm_iou=0.45):
    """One image through maf_pr_match with native-space xyxy labels (no rescale) -> int16 masks [n] on the device."""
    _on_device(detections, labels)
    dev = detections.device
    n, m = int(detections.shape[0]), int(labels.shape[0])
    if n > lib.PR_MAX_DET or m > lib.PR_MAX_LABELS:
        raise lib.MafError("metrics supports <= %d detections and <= %d labels per image" % (lib.PR_MAX_DET, lib.PR_MAX_LABELS))
    rows = detections.float().contiguous().reshape(1, n, 6)
    count = torch.full((1,), n, dtype=torch.int32, device=dev)
    targets = torch.cat([torch.zeros(m, 1, device=dev), labels.float().reshape(m, 5)], 1).contiguous()
    offs = torch.zeros(2, dtype=torch.int64, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    masks = torch.empty(n, dtype=torch.int16, device=dev)
    iouv = _iouv_dev(iouv, dev)
    _check(lib.load().maf_pr_match(rows.data_ptr(), count.data_ptr(), 1, n, targets.data_ptr() if m else None, m, None, 1, 1, iouv.data_ptr(),
                                   iouv.numel(), nc, flags | lib.PR_LABELS_XYXY, cm_conf, cm_iou, offs.data_ptr(), offs.data_ptr() + 8,
                                   keys.data_ptr(), masks.data_ptr(), n, state.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return masks, iouv.numel()


def process_batch(detections, labels, iouv=None, nc=lib.PR_MAX_CLASSES):
    """metrics.py:145-167: detections [N, 6] (x1, y1, x2, y2, conf, class), labels [M, 5] (class, x1, y1, x2, y2), both native pixels, on the
    device -> bool [N, len(iouv)] on the device.  Classes must be integers in [0, nc)."""
    _on_device(detections, labels)
    niou = len(default_iouv() if iouv is None else iouv)
    n = int(detections.shape[0])
    if n == 0 or labels.shape[0] == 0:
        return torch.zeros(n, niou, dtype=torch.bool, device=detections.device)
    state = torch.zeros(lib.load().maf_pr_state_ints(nc), dtype=torch.int32, device=detections.device)
    masks, niou = _match_one(detections, labels, iouv, nc, 0, state)
    bits = torch.arange(niou, device=detections.device, dtype=torch.int32)
    return ((masks.int()[:, None] >> bits) & 1).bool()


class ConfusionMatrix:
    """metrics.py:169-224 on the device: process_batch(detections, labels) accumulates without a host sync; matrix (float64 numpy
    [nc + 1, nc + 1], as the reference's) and tp_fp() copy it back."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        if not 0 < nc <= lib.PR_MAX_CLASSES:
            raise lib.MafError("ConfusionMatrix supports 1..%d classes, got %d" % (lib.PR_MAX_CLASSES, nc))
        self.nc, self.conf, self.iou_thres = int(nc), float(conf), float(iou_thres)
        self._state = None

    def process_batch(self, detections, labels):
        _on_device(detections, labels)
        if self._state is None:
            self._state = torch.zeros(lib.load().maf_pr_state_ints(self.nc), dtype=torch.int32, device=detections.device)
        if detections.shape[0] == 0 or labels.shape[0] == 0:
            if labels.shape[0] and detections.shape[0] == 0:  # no detection above conf: every label is background
                cls = labels[:, 0].long()
                self._state[2 + 2 * self.nc:].view(self.nc + 1, self.nc + 1)[self.nc].index_add_(
                    0, cls, torch.ones_like(cls, dtype=torch.int32))
            return
        _match_one(detections, labels, None, self.nc, lib.PR_CONFUSION, self._state, self.conf, self.iou_thres)

    @property
    def matrix(self):
        if self._state is None:
            return np.zeros((self.nc + 1, self.nc + 1))
        s = self._state.cpu().numpy()
        if s[0]:
            raise lib.MafError("ConfusionMatrix: %s" % _error_text(int(s[0])))
        return s[2 + 2 * self.nc:].reshape(self.nc + 1, self.nc + 1).astype(np.float64)

    def tp_fp(self):
        m = self.matrix
        tp = m.diagonal()
        fp = m.sum(1) - tp
        return tp[:-1], fp[:-1]


def _desc_bits(conf):
    """The sort key's low word: order-preserving bits of fp32 conf, complemented (ascending key = descending conf); as pr_metric.hip."""
    u = (conf.float() + 0.0).view(torch.int32).long() & 0xFFFFFFFF
    ordered = torch.where(u >= 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    return (~ordered) & 0xFFFFFFFF


def ap_per_class(tp, conf, pred_cls, target_cls, plot=False, save_dir=".", names=()):
    """metrics.py:13-75 on device tensors -> (p, r, ap, f1, ap_class) as NumPy arrays, rows per np.unique(target_cls).  Equal confidences
    keep their input order.  plot=True raises: drawing is the caller's."""
    if plot:
        raise lib.MafError("ap_per_class(plot=True): plotting is not part of this package; draw p / r / f1 / py from PrMetric's result")
    _on_device(tp, conf, pred_cls, target_cls)
    dev = conf.device
    tp = tp.reshape(conf.numel(), -1)
    niou = tp.shape[1]
    if not 0 < niou <= 16:
        raise lib.MafError("ap_per_class takes 1..16 thresholds, got %d" % niou)
    pcls, tcls = pred_cls.reshape(-1).long(), target_cls.reshape(-1).long()
    nc = int(torch.cat([pcls, tcls, torch.zeros(1, dtype=torch.long, device=dev)]).max().item()) + 1
    if nc > lib.PR_MAX_CLASSES or (tcls.numel() and int(tcls.min().item()) < 0) or (pcls.numel() and int(pcls.min().item()) < 0):
        raise lib.MafError("ap_per_class: classes must lie in [0, %d)" % lib.PR_MAX_CLASSES)
    keys = (pcls << 32) | _desc_bits(conf.reshape(-1))
    masks = (tp.to(torch.int32) << torch.arange(niou, device=dev, dtype=torch.int32)).sum(1).to(torch.int16)
    state = torch.zeros(lib.load().maf_pr_state_ints(nc), dtype=torch.int32, device=dev)
    state[1] = tp.any().int()
    state[2:2 + nc] = torch.bincount(tcls, minlength=nc).int()
    state[2 + nc:2 + 2 * nc] = torch.bincount(pcls, minlength=nc).int()
    if keys.numel() == 0:
        keys, masks = torch.full((1,), INT64_MAX, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int16, device=dev)
    h = _curves(keys.contiguous(), masks.contiguous(), state, nc, niou).cpu().numpy()
    parts = _split(h, nc, niou)
    present = parts["nt"] > 0
    return parts["p"][present], parts["r"][present], parts["ap"][present], parts["f1"][present], np.nonzero(present)[0].astype(np.int32)
