"""The convergence run on procedural data (data.SyntheticShapes): a train split rendered into a data.ResidentSplit, the real
Trainer (bf16 products, device draws, mask-weighted rays) for a step budget, then evaluate(metrics="device") on held-out objects
of the test stage — PSNR / SSIM against the all-white frame's PSNR (the trivial predictor), the depth error against the ray
cast's own depth — and one sweep of evaluate(occupancy={"sigma_thresh": ...}) on the trained net: share of hit rays and PSNR
change per threshold.  Writes profiles/synthetic_convergence.txt.  A tool, not a test: no figure of it is an acceptance
condition.
    python tools/train_synthetic.py --steps 1500"""
import argparse
import contextlib
import io
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as gu  # noqa: E402
from hip_util import model_conf  # noqa: E402


def white_psnr(item, targets):
    """Mean over the target views of the PSNR of an all-white frame against the view, images in [0, 1]: evaluate's averaging."""
    gt = item["images"][targets].float() / 255.0
    mse = ((1.0 - gt) ** 2).mean(dim=(1, 2, 3)).double()
    return float((10.0 * torch.log10(1.0 / mse)).mean())


def depth_error(out_dir, dataset, targets, z_near, z_far):
    """Mean |rendered depth - ray-cast depth| over the foreground pixels (finite ground truth) of every target view."""
    total, count = 0.0, 0
    for i in range(len(dataset)):
        item = dataset[i]
        for v in targets:
            norm = np.load(os.path.join(out_dir, os.path.basename(item["path"]), f"{v:06d}_depth.npy"))
            gt = item["depth"][v].numpy()
            fg = np.isfinite(gt)
            total += float(np.abs(norm[fg] * (z_far - z_near) + z_near - gt[fg]).sum())
            count += int(fg.sum())
    return total / max(count, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--test-objects", type=int, default=8)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1500, help="training steps (rounded up to whole epochs)")
    ap.add_argument("--sb", type=int, default=4)
    ap.add_argument("--rays", type=int, default=128)
    ap.add_argument("--nviews", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--prop-inside", type=float, default=0.5, help="share of rays on the mask's foreground; negative: box draws")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "bf16x3"])
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.5, 2.0, 5.0, 10.0, 20.0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synthetic_convergence.txt"))
    a = ap.parse_args()

    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet, evalio, train
    from pixel_nerf_multiscale_amd.data import ResidentSplit, get_split_dataset
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    from pixel_nerf_multiscale_amd.render import occupancy as occ
    dev = torch.device("cuda")
    common = dict(n_objects=a.objects, n_test=a.test_objects, n_views=a.views, image_size=a.size, seed=a.seed)
    train_set = get_split_dataset("synthetic", None, want_split="train", as_bytes=True, **common)
    train_set[0]                                                   # the first launch: code objects, the pinned blocks
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pool = ResidentSplit(train_set, dev, device_boxes=True, device_masks=True)
    torch.cuda.synchronize()
    t_pool = time.perf_counter() - t0

    torch.manual_seed(a.seed)
    net = PixelNeRFNet(model_conf(dict(gu.CASES["full_ns1"]), "fp32")).cuda()
    net.train_precision = a.precision
    rend = NeRFRenderer(n_coarse=64, n_fine=32, n_fine_depth=16, white_bkgd=True).cuda()
    per_epoch = a.objects // a.sb
    epochs = max(1, math.ceil(a.steps / per_epoch))
    never = 10 ** 9
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"synthetic convergence run: seed {a.seed}, {a.objects} train objects x {a.views} views of {a.size} x {a.size} (ss 2, up to 4 "
        f"primitives), SB {a.sb}, {a.rays} rays per object, nviews {a.nviews}, prop_inside {a.prop_inside}, lr {a.lr}, {a.precision}, "
        f"n_coarse 64 / n_fine 32 + 16, {epochs} epochs of {per_epoch} steps")
    say(f"pool: {pool.nbytes / 1e6:.1f} MB generated in {t_pool:.2f} s ({a.objects * a.views / t_pool:.0f} views/s, one launch and one "
        "copy back per object)")
    with tempfile.TemporaryDirectory() as tmp:
        t = train.Trainer(net, rend, pool, None, name="synthetic", checkpoints_path=os.path.join(tmp, "ckpt"),
                          logs_path=os.path.join(tmp, "logs"), batch_size=a.sb, ray_batch_size=a.rays, nviews=a.nviews,
                          loss=RenderLoss(1.0, 1.0), num_epochs=epochs, lr=a.lr, draws="device", seed=a.seed,
                          prop_inside=a.prop_inside if a.prop_inside >= 0 else None,
                          print_interval=never, save_interval=never, eval_interval=never, vis_interval=never)
        log = io.StringIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for epoch in range(epochs):
            with contextlib.redirect_stdout(log):
                t.train_epoch(epoch)
            print(f"epoch {epoch + 1} / {epochs}: {time.perf_counter() - t0:.1f} s", flush=True)
        torch.cuda.synchronize()
        t_train = time.perf_counter() - t0
        losses = [float(l.split("avg_loss=")[1]) for l in log.getvalue().splitlines() if "avg_loss=" in l]
        marks = sorted({0, len(losses) // 4, len(losses) // 2, 3 * len(losses) // 4, len(losses) - 1})
        say(f"training: {t.global_step} steps in {t_train:.1f} s = {t.global_step / t_train:.2f} steps/s (the first epoch's warm-up "
            f"included), {int(t.optimizer.step_count)} applied and {int(t.optimizer.skipped)} skipped by the optimiser; mean loss of "
            "epoch " + ", ".join(f"{e}: {losses[e]:.4f}" for e in marks))

        net.eval()
        test_f = get_split_dataset("synthetic", None, want_split="test", as_bytes=False, **common)
        test_b = get_split_dataset("synthetic", None, want_split="test", as_bytes=True, want_depth=True, **common)
        targets = list(range(1, a.views))
        kw = dict(source="0", verbose=False, seed=a.seed + 1, metrics="device", max_objects=len(test_f))
        base = os.path.join(tmp, "eval")
        psnr, ssim, count = evalio.evaluate(net, rend, test_f, base, write_depth=True, **kw)
        white = float(np.mean([white_psnr(test_b[i], targets) for i in range(len(test_b))]))
        say(f"held-out: {count} objects of the test stage, source view 0, {len(targets)} target views each: PSNR {psnr:.2f} dB, "
            f"SSIM {ssim:.4f}; the all-white frame scores PSNR {white:.2f} dB on the same views")
        say(f"depth: mean |rendered - ray cast| on foreground pixels {depth_error(base, test_b, targets, test_f.z_near, test_f.z_far):.4f} "
            f"(scene radius 0.5, cameras at 1.3; the ground truth is taken at the pixel's first sub-sample)")

        seen, real = [], occ.read_counts

        def spy(counts):
            out = real(counts)
            seen.extend(out)
            return out

        occ.read_counts = spy
        try:
            for thresh in a.thresholds:
                del seen[:]
                p, s, _ = evalio.evaluate(net, rend, test_f, os.path.join(tmp, f"occ_{thresh}"), **kw,
                                          occupancy=dict(sigma_thresh=thresh, c1=(-0.6, -0.6, -0.6), c2=(0.6, 0.6, 0.6), reso=64))
                share = sum(seen) / (len(seen) * a.size * a.size) if seen else float("nan")
                say(f"occupancy sigma_thresh {thresh:g} (box +-0.6, 64^3 samples): {100 * share:.1f} % of the rays hit, PSNR {p:.2f} dB "
                    f"({p - psnr:+.2f}), SSIM {s:.4f} ({s - ssim:+.4f})")
        finally:
            occ.read_counts = real
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
