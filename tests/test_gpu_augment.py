"""-m gpu: the training augmentation on the device (csrc/augment.hip, maf-yolo_amd/augment.py).

* train_batch equals the NumPy restatement (tests/augment_ref.py) bit for bit over many seeds: the MAF-YOLO-n hyp, the non-mosaic branch
  (letterbox's second resize included), mixup on every sample, both flips, HSV off; frames of odd widths, sizes above and below 640, long
  sides that load_image rounds to 639, cropped views with a row pitch; B up to 70;
* the C-ABI, the torch op and train_batch give the same bytes;
* end to end: train_batch's batch feeds Model (train) + ComputeLoss + one SGD step, with the same finite loss as the restatement's batch;
* train_batch makes no device -> host synchronisation.
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import augment_ref as R
import maf_yolo_amd as M
from maf_yolo_amd import augment as A
from maf_yolo_amd import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HYP_N = dict(hsv_h=0.015, hsv_s=0.7, hsv_v=0.4, degrees=0.0, translate=0.1, scale=0.5, shear=0.0, flipud=0.0, fliplr=0.5,
             mosaic=1.0, mixup=0.0, dy_label=5, dy_mixup=0.2, mask_refine=True, copy_paste=0.05)
HYPS = {
    "default": HYP_N,
    "nomosaic": dict(HYP_N, mosaic=0.0, dy_mixup=0.0),
    "mixup_flips": dict(HYP_N, mixup=1.0, flipud=0.5, degrees=7.0, shear=3.0),
    "no_hsv_flips": dict(HYP_N, hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, flipud=1.0, fliplr=1.0, translate=0.0, scale=0.0),
}
SIZES = [(480, 640), (640, 640), (77, 61), (1080, 1920), (303, 201), (1, 1), (720, 1280), (638, 17), (1280, 1280), (333, 501), (612, 459),
         (17, 638), (640, 427)]


def _dataset(seed, n_img=24, img_size=640):
    rs = np.random.RandomState(seed)
    sizes = list(SIZES)
    while len(sizes) < n_img:
        sizes.append((int(rs.randint(16, 1500)), int(rs.randint(16, 1500))))
    labels = []
    for _ in sizes:
        n = int(rs.randint(0, 8))
        labels.append(np.concatenate([rs.randint(0, 80, (n, 1)), rs.uniform(0.1, 0.9, (n, 2)), rs.uniform(0.05, 0.5, (n, 2))], 1).astype(np.float32))
    host = [R.synth_frame(h, w, seed * 100 + i) for i, (h, w) in enumerate(sizes)]
    frames = []
    for i, f in enumerate(host):
        if i % 3 == 1:                                        # a cropped view: rows with a pitch wider than 3 w
            big = np.zeros((f.shape[0] + 3, f.shape[1] + 5, 3), np.uint8)
            big[2:2 + f.shape[0], 3:3 + f.shape[1]] = f
            frames.append(torch.from_numpy(big).to(DEV)[2:2 + f.shape[0], 3:3 + f.shape[1]])
        else:
            frames.append(torch.from_numpy(f).to(DEV))
    return sizes, labels, host, frames


def _want(aug, samples, host):
    staged = R.staged_frames(aug, samples, dict(enumerate(host)))
    return np.stack([R.sample_pixels(aug, smp, staged) for smp in samples])


def _draw(aug, B, seed):
    random.seed(seed)
    np.random.seed(seed)
    return aug.draw_batch(np.random.RandomState(seed).randint(0, len(aug), B))


@pytest.mark.parametrize("name", list(HYPS))
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_train_batch_equals_restatement(name, seed):
    sizes, labels, host, frames = _dataset(seed)
    aug = A.TrainAugment(labels, sizes, HYPS[name], 640)
    samples = _draw(aug, 6, seed)
    imgs, targets = M.train_batch(frames, samples, aug)
    assert imgs.dtype == torch.uint8 and tuple(imgs.shape) == (6, 3, 640, 640) and imgs.device == DEV
    got = imgs.cpu().numpy()
    want = _want(aug, samples, host)
    for b in range(6):
        assert np.array_equal(got[b], want[b]), (name, seed, b, int((got[b] != want[b]).sum()))
    rows = np.concatenate([np.concatenate([np.full((len(s.labels), 1), b, np.float32), s.labels.astype(np.float32)], 1) for b, s in
                           enumerate(samples)], 0).reshape(-1, 6)
    assert targets.dtype == torch.float32 and np.array_equal(targets.cpu().numpy(), rows)


def test_branches_are_exercised():
    sizes, labels, host, frames = _dataset(4)
    aug = A.TrainAugment(labels, sizes, HYPS["mixup_flips"], 640)
    samples = _draw(aug, 24, 4)
    assert all(len(s.layers) == 2 for s in samples) and any(s.flipud for s in samples) and any(s.fliplr for s in samples)
    aug = A.TrainAugment(labels, sizes, HYPS["nomosaic"], 640)
    samples = aug.draw_batch(range(len(sizes)))
    assert any(t.frame[0] == "lb" for s in samples for t in s.layers[0].tiles), "no frame took letterbox's second resize"
    imgs, _ = M.train_batch(frames, samples, aug)
    assert np.array_equal(imgs.cpu().numpy(), _want(aug, samples, host))


@pytest.mark.parametrize("img_size", [320, 416])
def test_other_image_sizes(img_size):
    sizes, labels, host, frames = _dataset(5)
    aug = A.TrainAugment(labels, sizes, HYPS["mixup_flips"], img_size)
    samples = _draw(aug, 5, 5)
    imgs, _ = M.train_batch(frames, samples, aug)
    assert tuple(imgs.shape) == (5, 3, img_size, img_size)
    assert np.array_equal(imgs.cpu().numpy(), _want(aug, samples, host))


def test_batch_of_70():
    sizes, labels, host, frames = _dataset(6, n_img=40)
    aug = A.TrainAugment(labels, sizes, dict(HYP_N, dy_mixup=0.5), 640)
    samples = _draw(aug, 70, 6)
    imgs, targets = M.train_batch(frames, samples, aug)
    got = imgs.cpu().numpy()
    want = _want(aug, samples, host)
    assert np.array_equal(got, want)
    assert int(targets[:, 0].max().item()) <= 69


def test_c_abi_torch_op_and_train_batch_agree():
    sizes, labels, host, frames = _dataset(7)
    aug = A.TrainAugment(labels, sizes, HYPS["mixup_flips"], 640)
    samples = _draw(aug, 4, 7)
    via_batch, _ = M.train_batch(frames, samples, aug)
    table, dev, keep = A.stage_batch(frames, samples, aug)
    table_dev = table.to(DEV)
    from maf_yolo_amd import torch_ops
    via_op = torch_ops.load().mosaic_affine(table, table_dev, 640)
    via_abi = torch.empty(4, 3, 640, 640, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    lib.check(lib.load().maf_mosaic_affine(C.c_void_p(table.data_ptr()), C.c_void_p(table_dev.data_ptr()), 4, 640, C.c_void_p(via_abi.data_ptr()), st))
    torch.cuda.synchronize()
    del keep
    assert torch.equal(via_op, via_batch) and torch.equal(via_abi, via_batch)


def test_rejects_cpu_and_wrong_frames():
    sizes, labels, host, frames = _dataset(8)
    aug = A.TrainAugment(labels, sizes, HYP_N, 640)
    samples = _draw(aug, 2, 8)
    with pytest.raises(M.MafError, match="CUDA"):
        M.train_batch([torch.from_numpy(f) for f in host], samples, aug)
    with pytest.raises(M.MafError, match="uint8"):
        M.train_batch([f.float() for f in frames], samples, aug)
    bad = list(frames)
    for i in A.needed_frames(samples):
        bad[i] = frames[i][:-1] if frames[i].shape[0] > 1 else frames[i][:, :0]
    with pytest.raises(M.MafError):
        M.train_batch(bad, samples, aug)


def test_end_to_end_training_step():
    """train_batch -> Model (train) + ComputeLoss + one SGD step: finite, and the same loss as the restatement's batch."""
    sizes, labels, host, frames = _dataset(9)
    aug = A.TrainAugment(labels, sizes, HYP_N, 640)
    samples = _draw(aug, 4, 9)
    imgs, targets = M.train_batch(frames, samples, aug)
    want = torch.from_numpy(_want(aug, samples, host)).to(DEV)
    losses = []
    for batch in (imgs, want):
        torch.manual_seed(0)
        m = M.Model("n").to(DEV).train()
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.937, nesterov=True)
        crit = M.ComputeLoss(ori_img_size=640, warmup_epoch=0)
        x = batch.float() / 255                                  # engine.py prepro_data
        feats, cls, reg = m(x)[0]
        loss, _ = crit((feats, cls, reg), targets, 0, 0)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    assert torch.isfinite(losses[0]).all() and torch.equal(losses[0], losses[1])


def test_no_host_sync():
    sizes, labels, host, frames = _dataset(10)
    aug = A.TrainAugment(labels, sizes, HYPS["mixup_flips"], 640)
    M.train_batch(frames, _draw(aug, 4, 10), aug)              # warm: op library loaded, pinned pool primed
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        imgs, targets = M.train_batch(frames, np.arange(8) % len(sizes), aug)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert tuple(imgs.shape) == (8, 3, 640, 640) and targets.shape[1] == 6
