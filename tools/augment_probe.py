"""Measurements of the training augmentation (csrc/augment.hip) on the GPU; prints ONE JSON line.

    python tools/augment_probe.py [--iters N] [--no-torch] [--polygons]

* bs 32 x 640^2 with the MAF-YOLO-n hyp (and a dy_mixup = 1 variant, mixup on most samples): a pool of decoded frames (1080p, 720p and
  480 x 640; > 256 MiB, so the reads come from HBM, not the Infinity Cache) that the batches' draws rotate through.  Per batch: event time of
  train_batch's device work (the resize launch + maf_mosaic_affine) and its host time; the bytes (frames read by the resizes, staging written
  and read back by the tile windows the warp touches, 1.2 MB of output per image).  Kernel times proper come from a rocprofv3 --kernel-trace
  --stats run of this same script (kernels `augment_resize_kernel` and `mosaic_affine_kernel`);
* the same warp / mixup / HSV / flip rule composed of torch ops on the GPU (gathers + integer arithmetic on the staged frames), timed as the
  baseline and compared bit for bit with the kernel;
* --polygons: polygon labels with MAF-YOLO-m's hyp (copy_paste 0.2) instead: per batch the event time of train_batch with the pasted
  contours (maf_polygon_mask + maf_mosaic_affine_paste), of the SAME draws with the contours removed (maf_mosaic_affine), and of the
  maf_polygon_mask launch alone; the masks' bytes (C^2 / 8 per pasted layer, written once and read by the taps).
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import maf_yolo_amd as M  # noqa: E402
from maf_yolo_amd import augment as A  # noqa: E402

DEV = torch.device("cuda:0")
HYP_N = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, flipud=0.0, fliplr=0.5,
             mosaic=1.0, mixup=0.0, dy_label=5, dy_mixup=0.2, mask_refine=True, copy_paste=0.05)


def pool(n):
    """n decoded frames on the device, sizes cycling 1080p / 720p / 480 x 640 (seeded noise: every byte value in play)."""
    sizes = [(1080, 1920), (720, 1280), (480, 640)]
    g = torch.Generator(device=DEV).manual_seed(0)
    frames, shapes, labels = [], [], []
    rs = np.random.RandomState(0)
    for i in range(n):
        h, w = sizes[i % 3]
        frames.append(torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device=DEV, generator=g))
        shapes.append((h, w))
        k = int(rs.randint(0, 12))
        labels.append(np.concatenate([rs.randint(0, 80, (k, 1)), rs.uniform(0.1, 0.9, (k, 2)), rs.uniform(0.05, 0.5, (k, 2))], 1).astype(np.float32))
    return frames, shapes, labels


def batch_bytes(aug, samples):
    """Resize reads (whole frames) + staging writes + the staging windows the tiles expose + the output."""
    s = aug.img_size
    read = staged = 0
    for i in A.needed_frames(samples):
        h0, w0 = aug.shapes[i]
        h, w = aug.loaded_hw(i)
        if (h, w) != (h0, w0):
            read += 3 * h0 * w0
            staged += 3 * h * w
    windows = sum(3 * (t.x1 - t.x0) * (t.y1 - t.y0) for smp in samples for layer in smp.layers for t in layer.tiles)
    return read + 2 * staged, windows, 3 * s * s * len(samples)


def torch_rule(table_samples, staged, aug):
    """The kernel's rule as torch ops: materialised canvas per layer, fixed-point taps, double blend, uint8 HSV, flips."""
    s = aug.img_size
    outs = []
    x = torch.arange(s, device=DEV, dtype=torch.float64)
    f = torch.arange(32, device=DEV)
    sdiv = torch.where(f.new_tensor(range(256)) > 0, torch.round((255 << 12) / torch.arange(256, device=DEV).clamp(min=1).double()), 0).long()
    hdiv = torch.where(f.new_tensor(range(256)) > 0, torch.round((180 << 12) / (6.0 * torch.arange(256, device=DEV).clamp(min=1).double())), 0).long()
    for smp in table_samples:
        imgs = []
        for layer in smp.layers:
            m = A.invert_affine(layer.M)
            size = 2 * s
            c = torch.full((size + 2, size + 2, 3), 114, dtype=torch.int64, device=DEV)
            for t in layer.tiles:
                fr = staged[t.frame]
                c[t.y0 + 1:t.y1 + 1, t.x0 + 1:t.x1 + 1] = fr[t.y0 + t.dy:t.y1 + t.dy, t.x0 + t.dx:t.x1 + t.dx].long()
            ad, bd = torch.round(m[0] * x * 1024).long(), torch.round(m[3] * x * 1024).long()
            X0, Y0 = torch.round((m[1] * x + m[2]) * 1024).long() + 16, torch.round((m[4] * x + m[5]) * 1024).long() + 16
            X, Y = (X0[:, None] + ad[None]) >> 5, (Y0[:, None] + bd[None]) >> 5
            sx, sy, fx, fy = (X >> 5).clamp(-32768, 32767), (Y >> 5).clamp(-32768, 32767), X & 31, Y & 31
            w = torch.stack([(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32], -1)

            def tap(a, b):
                return c[(b + 1).clamp(0, size + 1), (a + 1).clamp(0, size + 1)]
            acc = tap(sx, sy) * w[..., :1] + tap(sx + 1, sy) * w[..., 1:2] + tap(sx, sy + 1) * w[..., 2:3] + tap(sx + 1, sy + 1) * w[..., 3:]
            imgs.append((acc + (1 << 14)) >> 15)
        img = imgs[0] if len(imgs) == 1 else (imgs[0].double() * smp.mix_r + imgs[1].double() * (1 - smp.mix_r)).long()
        if smp.lut is not None:
            lut = torch.from_numpy(smp.lut.astype(np.int64)).to(DEV)
            b, g, r = img[..., 0], img[..., 1], img[..., 2]
            v = torch.maximum(torch.maximum(b, g), r)
            diff = v - torch.minimum(torch.minimum(b, g), r)
            sat = (diff * sdiv[v] + 2048) >> 12
            h = torch.where(v == r, g - b, torch.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
            h = (h * hdiv[diff] + 2048) >> 12
            h = torch.where(h < 0, h + 180, h)
            h, sat, v = lut[0][h], lut[1][sat], lut[2][v]
            hf = torch.fmod(h.float() * np.float32(np.float32(6) / np.float32(180)), 6.0)
            sf = sat.float() * np.float32(np.float32(1) / np.float32(255))
            vf = v.float()
            sec = torch.floor(hf)
            hf = hf - sec
            sec = sec.long().clamp(0, 5)
            tab = torch.stack([vf, vf * (1 - sf), vf * (1 - sf * hf), vf * (1 - sf * (1 - hf))], -1)
            sd = torch.tensor([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]], device=DEV)
            bgr = torch.gather(tab, -1, sd[sec])
            bgr = torch.where((sf == 0)[..., None], vf[..., None], bgr)
            img = torch.round(bgr).clamp(0, 255).long()
        if smp.flipud:
            img = img.flip(0)
        if smp.fliplr:
            img = img.flip(1)
        outs.append(img.permute(2, 0, 1).flip(0).to(torch.uint8))
    return torch.stack(outs)


def polygon_pool(shapes, seed=0):
    """Seeded polygon labels for the pool: 3..11 polygons of 6..40 vertices per image and the boxes the label reader derives from them."""
    rs = np.random.RandomState(seed)
    labels, segments = [], []
    for _ in shapes:
        segs, rows = [], []
        for _ in range(int(rs.randint(3, 12))):
            k = int(rs.randint(6, 41))
            c, rad = rs.uniform(0.15, 0.85, 2), rs.uniform(0.03, 0.25, 2)
            ang = np.sort(rs.uniform(0, 2 * np.pi, k))
            xy = np.stack([c[0] + rad[0] * np.cos(ang), c[1] + rad[1] * np.sin(ang)], 1).clip(0, 1).astype(np.float32)
            segs.append(xy)
            lo, hi = xy.min(0), xy.max(0)
            rows.append([float(rs.randint(0, 80)), (lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, hi[0] - lo[0], hi[1] - lo[1]])
        segments.append(segs)
        labels.append(np.array(rows, np.float32))
    return labels, segments


def _timed(fn, items):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in items]
    for (e0, e1), it in zip(ev, items):
        e0.record()
        fn(it)
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def polygons_case(args, frames, shapes):
    """train_batch with copy_paste's contours, the same draws without them, and the mask launch alone."""
    import copy
    from maf_yolo_amd import lib
    labels, segments = polygon_pool(shapes)
    hyp = dict(HYP_N, copy_paste=0.2, mixup=0.1, dy_mixup=0.4)                 # configs/MAF-YOLO-m.py
    aug = A.TrainAugment(labels, shapes, hyp, 640, segments=segments, polygons=True)
    random.seed(0)
    np.random.seed(0)
    rs = np.random.RandomState(1)
    batches = [aug.draw_batch(rs.randint(0, len(frames), args.bs)) for _ in range(args.iters)]
    plain = copy.deepcopy(batches)
    for b in plain:
        for smp in b:
            for layer in smp.layers:
                layer.paste = []
    staged = [A.stage_paste(b) for b in batches]
    L = lib.load()
    st = torch.cuda.current_stream(DEV).cuda_stream
    words = 1280 * 40
    n_max = max(p[1][0] for p in staged if p is not None)
    masks = torch.empty((n_max, words), dtype=torch.int32, device=DEV)
    tables = [(p[0], torch.from_numpy(p[0]).to(DEV), p[1]) for p in staged if p is not None]

    def mask_launch(t):
        tab, tab_dev, (n, npoly, nvert) = t
        lib.check(L.maf_polygon_mask(tab.ctypes.data, tab_dev.data_ptr(), n, npoly, nvert, 1280, masks.data_ptr(), st))
    for b, q in zip(batches[:3], plain[:3]):                                   # warm-up
        M.train_batch(frames, b, aug)
        M.train_batch(frames, q, aug)
    torch.cuda.synchronize()
    with_ms, without_ms = [], []
    for _ in range(2):                                                         # alternate the two versions: the host is shared
        with_ms += _timed(lambda b: M.train_batch(frames, b, aug), batches)
        without_ms += _timed(lambda b: M.train_batch(frames, b, aug), plain)
    mask_ms = _timed(mask_launch, tables)
    same = all(torch.equal(M.train_batch(frames, b, aug)[1], M.train_batch(frames, q, aug)[1]) for b, q in zip(batches[:2], plain[:2]))
    layers = [p[1][0] if p is not None else 0 for p in staged]
    return dict(train_batch_polygons_ms_median=round(statistics.median(with_ms), 4), train_batch_same_draws_no_paste_ms_median=round(statistics.median(without_ms), 4),
                polygon_mask_ms_median=round(statistics.median(mask_ms), 4), pasted_layers_per_batch=round(float(np.mean(layers)), 2),
                contours_per_batch=round(float(np.mean([p[1][1] if p is not None else 0 for p in staged])), 1),
                vertices_per_batch=round(float(np.mean([p[1][2] if p is not None else 0 for p in staged])), 1),
                mask_MB_per_batch=round(float(np.mean(layers)) * 1280 * 1280 / 8 / 1e6, 2), targets_equal=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch-ops baseline out (counter runs: only the kernels' dispatches)")
    ap.add_argument("--polygons", action="store_true", help="polygon labels: train_batch with and without copy_paste's contours on the same draws")
    args = ap.parse_args()
    frames, shapes, labels = pool(90)                          # 30 x (6.2 + 2.8 + 0.9) MB = 297 MB (283 MiB) of frames
    in_bytes = sum(f.numel() for f in frames)
    out = dict(bs=args.bs, img_size=640, pool_frames=len(frames), pool_MiB=round(in_bytes / 2 ** 20, 1), cases={})
    if args.polygons:
        out["cases"]["polygons_maf_yolo_m"] = polygons_case(args, frames, shapes)
        print(json.dumps(out))
        return
    for name, hyp in (("maf_yolo_n", HYP_N), ("dy_mixup_1", dict(HYP_N, dy_mixup=1.0, dy_label=100))):
        aug = A.TrainAugment(labels, shapes, hyp, 640)
        random.seed(0)
        np.random.seed(0)
        rs = np.random.RandomState(1)
        batches = [aug.draw_batch(rs.randint(0, len(frames), args.bs)) for _ in range(args.iters)]
        for b in batches[:3]:
            M.train_batch(frames, b, aug)                      # warm-up: op library, pinned pool
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in batches]
        host = []
        for (e0, e1), b in zip(ev, batches):
            e0.record()
            t0 = time.perf_counter()
            M.train_batch(frames, b, aug)
            host.append((time.perf_counter() - t0) * 1e3)
            e1.record()
        torch.cuda.synchronize()
        dev_ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        rb, win, ob = np.mean([batch_bytes(aug, b) for b in batches], 0)
        case = dict(device_ms_median=round(statistics.median(dev_ms), 4), host_ms_median=round(statistics.median(host), 3),
                    mixup_frac=round(float(np.mean([len(s.layers) == 2 for b in batches for s in b])), 3),
                    resize_MB=round(rb / 1e6, 1), tile_window_MB=round(win / 1e6, 1), out_MB=round(ob / 1e6, 1))
        if not args.no_torch:
            b = batches[0]
            staged = _staged_tensors(frames, b, aug)
            want = M.train_batch(frames, b, aug)[0]
            got = torch_rule(b, staged, aug)
            torch.cuda.synchronize()
            t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(3):
                torch_rule(b, staged, aug)
            t1.record()
            torch.cuda.synchronize()
            case["torch_ops_ms"] = round(t0.elapsed_time(t1) / 3, 2)
            case["torch_ops_bit_exact"] = bool(torch.equal(got, want))
        out["cases"][name] = case
    print(json.dumps(out))


def _staged_tensors(frames, samples, aug):
    """The staged frames of a batch as device tensors, one maf_augment_resize call per frame key (the torch baseline starts from these)."""
    from maf_yolo_amd import lib
    out = {}
    L = lib.load()
    st = torch.cuda.current_stream(DEV).cuda_stream
    for key in sorted({t.frame for smp in samples for layer in smp.layers for t in layer.tiles}, key=lambda k: (len(k), k)):
        i = key[1]
        h, w = aug.loaded_hw(i)
        if ("load", i) not in out:
            out[("load", i)] = frames[i] if (h, w) == aug.shapes[i] else _resize(L, st, frames[i], h, w)
        if key[0] == "lb":
            out[key] = _resize(L, st, out[("load", i)], key[3], key[2])
    return out


def _resize(L, st, f, nh, nw):
    from maf_yolo_amd import lib
    import ctypes as C
    dst = torch.empty(nh, nw, 3, dtype=torch.uint8, device=DEV)
    e = lib.MafAugmentFrame(src=f.data_ptr(), src_pitch=f.stride(0), h=f.shape[0], w=f.shape[1], dst=dst.data_ptr(), new_h=nh, new_w=nw)
    tab = torch.from_numpy(np.frombuffer(bytes(e), np.uint8).copy()).to(DEV)
    lib.check(L.maf_augment_resize(C.byref(e), tab.data_ptr(), 1, st))
    torch.cuda.synchronize()
    return dst


if __name__ == "__main__":
    main()
