"""train.Trainer end to end on the smallest configuration: the tiny MLP (d_hidden 32) behind the real encoder (three levels: a
16 x 16 image leaves a 2 x 2 map of 128 channels, the smallest the kernels take), an SRN tree of
4 objects x 3 views of 16 x 16 pixels written with data_trees, SB 2, 32 rays per object, nviews [1, 2], epochs of two steps,
fp32.  The runs that are compared bit for bit run with torch.backends.cudnn.deterministic = True (the encoder's convolutions
are the only part of a step that is not repeatable by construction)."""
import contextlib
import io
import os
import re
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import data_trees as dt
import golden_util as gu
from hip_util import model_conf

pytestmark = pytest.mark.gpu

W = H = 16
NV, SB, RAYS, NVIEWS = 3, 2, 32, [1, 2]


@pytest.fixture(autouse=True)
def _deterministic_convolutions():
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = was


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("srn")
    for stage, n_obj in (("train", 4), ("val", 2)):
        for o in range(n_obj):
            images = dt.boxed_views(NV, H, W, [(2 + v, 3, 12, 13 - v - o % 2) for v in range(NV)], seed=10 * o + (stage == "val"))
            poses = np.stack([gu.pose_spherical(40.0 * v + 13.0 * o, -20.0, 1.3) for v in range(NV)]).astype(np.float32)
            poses[:, :, 1:3] *= -1.0                        # stored in the OpenCV convention; the dataset flips it back
            dt.write_srn_object(str(root / f"cars_{stage}" / f"obj{o}"), images, poses, 16.5, 8.0, 8.0, ["000000", "000001", "000002"])
    return str(root / "cars")


def _datasets(tree, as_bytes=False):
    from pixel_nerf_multiscale_amd.data import get_split_dataset
    return (get_split_dataset("srn", tree, want_split="train", as_bytes=as_bytes),
            get_split_dataset("srn", tree, want_split="val", as_bytes=as_bytes))


def _model():
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet
    torch.manual_seed(0)
    conf = model_conf(dict(gu.CASES["tiny_ns2_codeview"]), "fp32")
    conf["encoder"]["num_layers"] = 3                       # 16 x 16 images: the third level is 2 x 2, the smallest map the kernels take
    net = PixelNeRFNet(conf).cuda()
    rend = NeRFRenderer(n_coarse=8, n_fine=6, n_fine_depth=2, white_bkgd=True).cuda()
    return net, rend


class Writer:
    def __init__(self):
        self.scalars, self.images = [], []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))

    def add_image(self, tag, img, step, dataformats="CHW"):
        self.images.append((tag, np.asarray(img), int(step), dataformats))


def _trainer(root, train_data, val_data, name="run", **kw):
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    net, rend = _model()
    conf = dict(name=name, checkpoints_path=os.path.join(root, "ckpt"), logs_path=os.path.join(root, "logs"), batch_size=SB,
                ray_batch_size=RAYS, nviews=NVIEWS, loss=RenderLoss(1.0, 1.0), num_epochs=2, print_interval=1, seed=5)
    conf.update(kw)
    return train.Trainer(net, rend, train_data, val_data, **conf)


def _state(t):
    torch.cuda.synchronize()
    return ({k: v.detach().clone() for k, v in t.net.state_dict().items()}, t.optimizer._exp_avg.clone(), t.optimizer._exp_avg_sq.clone(),
            int(t.optimizer.step_count), t.global_step)


def _assert_same(a, b):
    assert a[3] == b[3] and a[4] == b[4]
    assert sorted(a[0]) == sorted(b[0])
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------------------ one run
@pytest.fixture(scope="module")
def first_run(tree, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("first"))
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        writer, log = Writer(), io.StringIO()
        with contextlib.redirect_stdout(log):
            t = _trainer(root, *_datasets(tree), writer=writer, eval_interval=1, vis_interval=1)
            t.start()
    finally:
        torch.backends.cudnn.deterministic = was
    return root, t, writer, log.getvalue()


def test_a_run_writes_its_checkpoints_and_its_log(first_run):
    root, t, writer, log = first_run
    ckpt = os.path.join(root, "ckpt", "run")
    assert sorted(os.listdir(ckpt)) == ["_renderer", "best.pth", "epoch_0000.pth", "epoch_0001.pth", "latest.pth"]
    lines = [l for l in log.split("\n") if re.search(r"\] E \d+ B \d+ ", l)]
    assert len(lines) == 4 and t.global_step == 4 and t.batches_per_epoch == 2
    for line, (e, b) in zip(lines, ((0, 0), (0, 1), (1, 0), (1, 1))):
        assert re.match(rf"\[\d+\.\d\ds/it\] E {e} B {b} rc:\d+\.\d{{4}} rf:\d+\.\d{{4}} t:\d+\.\d{{4}} grad_norm:\d+\.\d{{4}} lr 0\.000100$", line), line
    latest = torch.load(os.path.join(ckpt, "latest.pth"), weights_only=False)
    epoch1 = torch.load(os.path.join(ckpt, "epoch_0001.pth"), weights_only=False)
    assert sorted(latest) == ["best_val_loss", "epoch", "global_step", "iter", "net_state_dict", "optimizer_state_dict", "seed"]
    assert (latest["epoch"], epoch1["epoch"], latest["global_step"], latest["seed"]) == (2, 1, 4, 5)
    assert sorted(torch.load(os.path.join(ckpt, "_renderer"), weights_only=False)) == ["iter_idx", "last_sched"]
    assert "Epoch 1 finished: avg_loss=" in log and "training finished" in log


def test_the_writer_gets_scalars_and_the_panel(first_run):
    root, t, writer, log = first_run
    tags = {s[0] for s in writer.scalars}
    assert {"train/t", "train/rc", "train/rf", "train/lr", "val/loss", "vis/psnr"} <= tags
    assert [s[2] for s in writer.scalars if s[0] == "train/t"] == [0, 1, 2, 3]
    assert [s[2] for s in writer.scalars if s[0] == "val/loss"] == [2, 4]
    vals = [s[1] for s in writer.scalars if s[0] == "val/loss"]
    assert all(np.isfinite(v) and v > 0 for v in vals) and t.best_val_loss == min(vals)
    best = torch.load(os.path.join(root, "ckpt", "run", "best.pth"), weights_only=False)
    assert best["best_val_loss"] == t.best_val_loss
    for e in (0, 1):
        img = np.asarray(Image.open(os.path.join(root, "logs", "run", "vis_%04d.png" % e)))
        assert img.dtype == np.uint8 and img.shape[0] == 2 * H and img.shape[1] in (5 * W, 6 * W) and img.shape[2] == 3
    assert len(writer.images) == 2 and writer.images[0][0] == "vis" and writer.images[0][3] == "HWC"
    assert np.array_equal(writer.images[1][1], np.asarray(Image.open(os.path.join(root, "logs", "run", "vis_0001.png"))))


def test_keep_last_one_leaves_one_epoch_file(first_run, tree, tmp_path):
    """A third epoch on top of the first run, resumed from its latest.pth, under keep_last_checkpoints = 1.  The resumed
    epoch 2 is an evaluation node of eval_interval = 2: start() validates before it trains, as the reference does."""
    root = str(tmp_path)
    shutil.copytree(os.path.join(first_run[0], "ckpt"), os.path.join(root, "ckpt"))
    writer = Writer()
    t = _trainer(root, *_datasets(tree), resume=True, num_epochs=3, keep_last_checkpoints=1, eval_interval=2, writer=writer)
    assert (t.epoch, t.global_step) == (2, 4) and t.best_val_loss == first_run[1].best_val_loss
    t.start()
    assert [s[2] for s in writer.scalars if s[0] == "val/loss"] == [4]
    files = sorted(os.listdir(os.path.join(root, "ckpt", "run")))
    assert files == ["_renderer", "best.pth", "epoch_0002.pth", "latest.pth"] and t.global_step == 6


# ------------------------------------------------------------------------------------------------------------ schedules
def test_boxes_are_switched_off_at_no_bbox_step(tree, tmp_path, monkeypatch):
    from pixel_nerf_multiscale_amd import util
    seen, real = [], util.train_draw

    def spy(bbox, *a, **kw):
        seen.append(None if bbox is None else bbox.clone())
        return real(bbox, *a, **kw)

    monkeypatch.setattr(util, "train_draw", spy)
    train_set, _ = _datasets(tree)
    t = _trainer(str(tmp_path), train_set, None, num_epochs=1, no_bbox_step=1)
    t.start()
    assert len(seen) == 2 and seen[0] is not None and seen[1] is None
    assert tuple(seen[0].shape) == (SB, NV, 4) and seen[0].is_cuda
    order = t._order.order[:SB]
    assert torch.equal(seen[0].cpu(), torch.stack([train_set[i]["bbox"] for i in order]))


def test_step_policy_halves_the_lr_at_the_epoch_boundary(tree, tmp_path):
    train_set, _ = _datasets(tree)
    t = _trainer(str(tmp_path), train_set, None, lr_policy="step", step_size=1, gamma=0.5)
    seen, real = [], t.train_step

    def step(data, global_step):
        out = real(data, global_step)
        seen.append((t.optimizer.param_groups[0]["lr"], float(t.optimizer.step_size) * (1.0 - 0.9 ** int(t.optimizer.step_count))))
        return out

    t.train_step = step
    t.start()
    assert [s[0] for s in seen] == [1e-4, 1e-4, 5e-5, 5e-5]
    for lr, used in seen:                                   # what the kernel applied: step_size = lr / (1 - beta1^t), fp32
        assert abs(used - lr) <= 1e-6 * lr
    ckpt = torch.load(os.path.join(str(tmp_path), "ckpt", "run", "latest.pth"), weights_only=False)
    # saved before the epoch's scheduler step, as the reference does; a resumed run steps the schedule up to its epoch
    assert "scheduler_state_dict" in ckpt and ckpt["optimizer_state_dict"]["param_groups"][0]["lr"] == 5e-5
    again = _trainer(str(tmp_path), train_set, None, lr_policy="step", step_size=1, gamma=0.5, resume=True, num_epochs=3)
    assert again.epoch == 2 and again.optimizer.param_groups[0]["lr"] == 2.5e-5


# ------------------------------------------------------------------------------------------------------------ reproducibility
def test_a_resumed_run_continues_bit_for_bit(tree, tmp_path):
    """Run A: two epochs.  Run B: one epoch, then a new Trainer on a freshly built net resumes from latest.pth for the second.
    Every entry of the net's state_dict, both moment buffers and the step count agree exactly."""
    train_set, val_set = _datasets(tree)
    a = _trainer(str(tmp_path / "a"), train_set, val_set)
    a.start()
    b1 = _trainer(str(tmp_path / "b"), train_set, val_set, num_epochs=1)
    b1.start()
    half = _state(b1)
    b2 = _trainer(str(tmp_path / "b"), train_set, val_set, resume=True)
    assert (b2.epoch, b2.global_step) == (1, 2)
    _assert_same(half, _state(b2))                          # the checkpoint holds everything a step reads
    b2.start()
    sa, sb = _state(a), _state(b2)
    assert sa[3] == 4 and sa[4] == 4
    _assert_same(sa, sb)
    assert not torch.equal(half[1], sa[1]) and any(not torch.equal(half[0][k], sa[0][k]) for k in half[0])


def test_resident_split_trains_like_the_loader(tree, tmp_path):
    """One epoch from a DataLoader over the as_bytes dataset and one from ResidentSplit(device_boxes=True): the same
    permutation, the same keys, the same parameters."""
    from pixel_nerf_multiscale_amd.data import ResidentSplit
    train_set, _ = _datasets(tree, as_bytes=True)
    a = _trainer(str(tmp_path / "loader"), train_set, None, num_epochs=1)
    a.start()
    split = ResidentSplit(train_set, "cuda", device_boxes=True)
    b = _trainer(str(tmp_path / "resident"), split, None, num_epochs=1)
    assert b.train_loader is None and b.batches_per_epoch == 2 and (b.z_near, b.z_far) == (0.8, 1.8)
    b.start()
    _assert_same(_state(a), _state(b))
    assert _state(a)[3] == 2
