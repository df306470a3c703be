"""train.Trainer(data_parallel=True) under two ranks, one process each, BOTH on cuda:0 over gloo (one card: RCCL refuses duplicate
devices; the code path is backend-agnostic torch.distributed).  ONE spawn runs every scenario — process start and the first
convolution dominate the time — on the tiny configuration of test_gpu_trainer.py: d_hidden 32 behind the real three-level
encoder, n_coarse 8 / n_fine 6 / n_fine_depth 2, an SRN tree of 4 training objects x 3 views of 16 x 16, batch_size 2 (one object
per rank), 32 rays per object, nviews [1, 2], 2 epochs of 2 steps, deterministic convolutions, device draws.

The encoder is frozen in the loop runs (freeze_enc=True) and in eval() in the step-level comparison: its BatchNorm would
otherwise normalise over the rank's own images, and a run would depend on the number of ranks by more than rounding.

Both ranks also create the two one-rank subgroups, so each runs the loop of one process in the same process, under the same
default group of two.  The file name sorts before test_00_ranks_on_one_card.py: this process must not initialise the GPU."""
import contextlib
import io
import os
import re
import socket
import sys
import traceback

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W = H = 16
NV, SB, RAYS, NVIEWS = 3, 2, 32, [1, 2]
GRAD_RTOL = 5e-4            # the project's gradient bound against the reference, per tensor, relative to max |g|
LOSS_RTOL = 1e-5            # what test_00_ranks_on_one_card.py allows between processes


def _write_tree(root):
    import data_trees as dt
    import golden_util as gu
    for stage, n_obj in (("train", 4), ("val", 2)):
        for o in range(n_obj):
            images = dt.boxed_views(NV, H, W, [(2 + v, 3, 12, 13 - v - o % 2) for v in range(NV)], seed=10 * o + (stage == "val"))
            poses = np.stack([gu.pose_spherical(40.0 * v + 13.0 * o, -20.0, 1.3) for v in range(NV)]).astype(np.float32)
            poses[:, :, 1:3] *= -1.0
            dt.write_srn_object(os.path.join(root, f"cars_{stage}", f"obj{o}"), images, poses, 16.5, 8.0, 8.0, ["000000", "000001", "000002"])
    return os.path.join(root, "cars")


def _model():
    import golden_util as gu
    from hip_util import model_conf
    from pixel_nerf_multiscale_amd import NeRFRenderer, PixelNeRFNet
    torch.manual_seed(0)
    conf = model_conf(dict(gu.CASES["tiny_ns2_codeview"]), "fp32")
    conf["encoder"]["num_layers"] = 3
    net = PixelNeRFNet(conf).cuda()
    rend = NeRFRenderer(n_coarse=8, n_fine=6, n_fine_depth=2, white_bkgd=True).cuda()
    return net, rend


class _Writer:
    def __init__(self):
        self.scalars, self.images = [], []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), int(step)))

    def add_image(self, tag, img, step, dataformats="CHW"):
        self.images.append((tag, int(step)))


def _trainer(root, sets, **kw):
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    net, rend = _model()
    conf = dict(name="run", checkpoints_path=os.path.join(root, "ckpt"), logs_path=os.path.join(root, "logs"), batch_size=SB,
                ray_batch_size=RAYS, nviews=NVIEWS, loss=RenderLoss(1.0, 1.0), num_epochs=2, print_interval=1, seed=5,
                freeze_enc=True)
    conf.update(kw)
    return train.Trainer(net, rend, sets[0], sets[1], **conf)


def _flat(t):
    torch.cuda.synchronize()
    return (torch.cat([p.detach().reshape(-1) for p in t.net.parameters()]).clone(), t.optimizer._exp_avg.clone(),
            t.optimizer._exp_avg_sq.clone())


def _step_level(rank, sets, out):
    """Scenario 1: the rank's object of a two-object batch with obj_base = rank and grad_hook = optim.allreduce, against the
    whole batch through a twin net with no hook, in the same process."""
    import torch.distributed as dist
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    from pixel_nerf_multiscale_amd.optim import DeviceAdam
    from pixel_nerf_multiscale_amd.parallel import frame_seed
    collate = torch.utils.data.default_collate
    whole, mine = collate([sets[0][0], sets[0][1]]), collate([sets[0][rank]])
    key = frame_seed(5, 0)
    kw = dict(ray_batch_size=RAYS, nviews=NVIEWS, z_near=sets[0].z_near, z_far=sets[0].z_far, loss=RenderLoss(1.0, 1.0),
              draws="device", seed=key)
    res = []
    for data, dp in ((mine, True), (whole, False)):
        net, rend = _model()
        net.train()
        net.encoder.eval()                                  # no batch statistics: an object's latents do not depend on its batch
        rend.train()
        params = [p for p in net.parameters() if p.requires_grad]
        optim = DeviceAdam(params, lr=1e-4)
        more = dict(grad_hook=optim.allreduce, obj_base=rank) if dp else {}
        with rend.keyed(key):
            ld = train.train_step(net, rend.bind_parallel(net, None), data, optim, **kw, **more)
        torch.cuda.synchronize()
        res.append((optim, ld))
    (opt_r, ld_r), (opt_w, ld_w) = res
    worst, n_moved = 0.0, 0
    for i, (a, b) in enumerate(zip(opt_r._slices, opt_w._slices)):
        scale = float(b.abs().max())
        err = float((a.double() / 2.0 - b.double()).abs().max())
        n_moved += scale > 0.0
        if scale > 0.0:
            worst = max(worst, err / scale)
        if err > GRAD_RTOL * scale:
            out.setdefault("grad_fail", []).append((i, err, scale))
    t_sum = ld_r["t"].detach().double().clone()
    dist.all_reduce(t_sum)
    out["step_grad_worst"], out["step_grad_tensors"] = worst, int(n_moved)
    out["step_t"] = (float(t_sum) / 2.0, float(ld_w["t"]), float(ld_r["t"]))
    out["step_norm"] = (float(opt_r.grad_norm), float(opt_w.grad_norm))
    out["step_count"] = (int(opt_r.step_count), int(opt_w.step_count), opt_r._grad_div)


def _worker(rank, world, port, root, tree, q):
    import datetime
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=240))
    out = {}
    try:
        from pixel_nerf_multiscale_amd.data import get_split_dataset
        solo_groups = [dist.new_group([r]) for r in range(world)]          # every rank creates every group, in one order
        solo = solo_groups[rank]
        torch.backends.cudnn.deterministic = True
        sets = (get_split_dataset("srn", tree, want_split="train"), get_split_dataset("srn", tree, want_split="val"))

        # the refusals, on every rank, before anything is allocated
        for kw, word in ((dict(batch_size=3), "does not divide"), (dict(draws="host"), "draws='device'")):
            try:
                _trainer(os.path.join(root, "refused"), sets, data_parallel=True, **kw)
                out.setdefault("not_refused", []).append(word)
            except ValueError as e:
                if word not in str(e):
                    out.setdefault("not_refused", []).append(str(e))
        out["refused_left_nothing"] = not os.path.exists(os.path.join(root, "refused"))

        _step_level(rank, sets, out)

        # A: the two-rank run
        saves, real_save = [], torch.save
        torch.save = lambda obj, f, *a, **k: (saves.append(os.path.basename(str(f))), real_save(obj, f, *a, **k))[1]
        writer, log = _Writer(), io.StringIO()
        try:
            with contextlib.redirect_stdout(log):
                a = _trainer(os.path.join(root, "A"), sets, data_parallel=True, eval_interval=1, vis_interval=1, writer=writer)
                init = _flat(a)[0]
                a.start()
        finally:
            torch.save = real_save
        fa = _flat(a)
        out["A"] = dict(world=a.world, rank=a.rank, obj_base=a.obj_base, rank_batch=a.rank_batch, global_step=a.global_step,
                        epoch=a.epoch, lr=a.optimizer.param_groups[0]["lr"], last_sched=int(a.renderer.last_sched),
                        best=a.best_val_loss, steps=int(a.optimizer.step_count), saves=len(saves), log=log.getvalue(),
                        scalars=list(writer.scalars), images=list(writer.images), batches_per_epoch=a.batches_per_epoch,
                        loader_len=len(a.train_loader))
        # 2: the ranks agree, bit for bit
        agree = []
        for x in fa + (torch.cat([b.reshape(-1).double() for b in a._state_buffers()]),):
            ref = x.clone()
            dist.broadcast(ref, 0)
            agree.append(bool(torch.equal(ref, x)))
        out["ranks_agree"] = agree                          # parameters, exp_avg, exp_avg_sq, the checkpointed buffers
        out["moved"] = not bool(torch.equal(fa[0], init))
        # the end-of-epoch broadcast of the buffers: a rank whose statistics drifted takes rank 0's
        bufs = a._state_buffers()
        probe = [next(b for b in bufs if b.dtype == torch.float32 and b.numel() > 1), next(b for b in bufs if b.dtype == torch.int64)]
        before = [b.clone() for b in probe]
        if rank == 1:
            for b in probe:
                b.add_(3)
        a._broadcast(bufs)
        out["buffers_follow_rank0"] = all(bool(torch.equal(b, c)) for b, c in zip(probe, before))

        with contextlib.redirect_stdout(io.StringIO()):
            # 3: one epoch, then a resumed second one, in the same group
            b1 = _trainer(os.path.join(root, "B"), sets, data_parallel=True, num_epochs=1)
            b1.start()
            b2 = _trainer(os.path.join(root, "B"), sets, data_parallel=True, resume=True)
            out["resumed_at"] = (b2.epoch, b2.global_step)
            b2.start()
            fb = _flat(b2)
            out["resume_same"] = all(bool(torch.equal(x, y)) for x, y in zip(fa, fb)) and int(b2.optimizer.step_count) == 4
            # 5: the same configuration as the loop of one process, under this rank's one-rank subgroup
            c = _trainer(os.path.join(root, f"C{rank}"), sets, data_parallel=solo, eval_interval=1)
            c.start()
            fc = _flat(c)
            val_a, val_c = a.validate(), c.validate()
        out["C"] = dict(world=c.world, rank=c.rank, global_step=c.global_step, epoch=c.epoch, lr=c.optimizer.param_groups[0]["lr"],
                        last_sched=int(c.renderer.last_sched), steps=int(c.optimizer.step_count),
                        files=sorted(os.listdir(os.path.join(root, f"C{rank}", "ckpt", "run"))))
        out["val"] = (val_a, val_c)
        out["distance"] = float((fa[0].double() - fc[0].double()).norm() / (fc[0].double() - init.double()).norm())
        out["max_param_diff"] = float((fa[0] - fc[0]).abs().max())
        # 6: a checkpoint of the two-rank run resumes under one rank, and trains on
        with contextlib.redirect_stdout(io.StringIO()):
            d = _trainer(os.path.join(root, f"D{rank}"), sets, data_parallel=solo, num_epochs=3,
                         resume=os.path.join(root, "A", "ckpt", "run", "latest.pth"))
            fd0 = _flat(d)
            out["D_loaded"] = (d.epoch, d.global_step, all(bool(torch.equal(x, y)) for x, y in zip(fa, fd0)),
                               int(d.renderer.last_sched))
            d.start()
        fd = _flat(d)
        out["D_done"] = (d.global_step, int(d.optimizer.step_count), bool(torch.isfinite(fd[0]).all()),
                         not bool(torch.equal(fd[0], fd0[0])),
                         "world_size" in torch.load(os.path.join(root, f"D{rank}", "ckpt", "run", "latest.pth"), weights_only=False))
        dist.barrier()
        q.put((rank, out))
    except Exception:
        out["error"] = traceback.format_exc()
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_train_one_global_batch(tmp_path):
    if torch.cuda.is_initialized():
        pytest.skip("this process has already initialised the GPU; worker processes must be started before that")
    import torch.multiprocessing as mp
    so = socket.socket()
    so.bind(("127.0.0.1", 0))
    port = so.getsockname()[1]
    so.close()
    os.environ["PYTHONPATH"] = os.pathsep.join([p for p in sys.path if p])
    root = str(tmp_path)
    tree = _write_tree(os.path.join(root, "srn"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, root, tree, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=600) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.terminate()
    for r in (0, 1):
        assert "error" not in res[r], res[r]["error"]
    assert all(p.exitcode == 0 for p in procs)

    for r in (0, 1):
        o = res[r]
        assert "not_refused" not in o and o["refused_left_nothing"]
        # 1: step level
        print(f"rank {r}: step gradients, worst per-tensor max|g_sum / 2 - g_whole| / max|g_whole| = {o['step_grad_worst']:.3e} over "
              f"{o['step_grad_tensors']} tensors (bound {GRAD_RTOL:.0e}); t all-reduced {o['step_t'][0]:.9g}, whole batch "
              f"{o['step_t'][1]:.9g}, this rank's own {o['step_t'][2]:.9g}")
        assert "grad_fail" not in o, o["grad_fail"][:5]
        assert o["step_grad_tensors"] >= 10
        t_ranks, t_whole, t_own = o["step_t"]
        assert abs(t_ranks - t_whole) <= LOSS_RTOL * abs(t_whole)
        assert abs(o["step_norm"][0] - o["step_norm"][1]) <= 1e-4 * o["step_norm"][1]       # the norm saw the divided gradient
        assert o["step_count"] == (1, 1, 1)
        a = o["A"]
        assert (a["world"], a["rank"], a["obj_base"], a["rank_batch"]) == (2, r, r, 1)
        assert (a["global_step"], a["epoch"], a["steps"], a["batches_per_epoch"], a["loader_len"]) == (4, 1, 4, 2, 2)
        # 2, 3
        assert o["ranks_agree"] == [True] * 4, o["ranks_agree"]
        assert o["moved"] and o["buffers_follow_rank0"]
        assert o["resumed_at"] == (1, 2) and o["resume_same"]
    assert res[0]["step_t"][2] != res[1]["step_t"][2]                                       # the ranks had different objects
    assert res[0]["A"]["best"] == res[1]["A"]["best"] and np.isfinite(res[0]["A"]["best"])

    # 4: one writer
    ckpt = os.path.join(root, "A", "ckpt", "run")
    assert sorted(os.listdir(ckpt)) == ["_renderer", "best.pth", "epoch_0000.pth", "epoch_0001.pth", "latest.pth"]
    assert res[1]["A"]["saves"] == 0 and res[0]["A"]["saves"] >= 8
    assert res[1]["A"]["log"] == "" and res[1]["A"]["scalars"] == [] and res[1]["A"]["images"] == []
    log = res[0]["A"]["log"]
    lines = [l for l in log.split("\n") if re.search(r"\] E \d+ B \d+ ", l)]
    assert len(lines) == 4
    for line, (e, b) in zip(lines, ((0, 0), (0, 1), (1, 0), (1, 1))):
        assert re.match(rf"\[\d+\.\d\ds/it\] E {e} B {b} rc:\d+\.\d{{4}} rf:\d+\.\d{{4}} t:\d+\.\d{{4}} grad_norm:\d+\.\d{{4}} lr 0\.000100$", line), line
    assert "Epoch 1 finished: avg_loss=" in log and "training finished" in log and "2 ranks of 1 objects" in log
    sc = res[0]["A"]["scalars"]
    assert [s[2] for s in sc if s[0] == "train/t"] == [0, 1, 2, 3] and [s[2] for s in sc if s[0] == "val/loss"] == [2, 4]
    assert res[0]["A"]["best"] == min(s[1] for s in sc if s[0] == "val/loss")
    assert [i[0] for i in res[0]["A"]["images"]] == ["vis", "vis"]
    assert sorted(f for f in os.listdir(os.path.join(root, "A", "logs", "run")) if f.startswith("vis_")) == ["vis_0000.png", "vis_0001.png"]
    latest = torch.load(os.path.join(ckpt, "latest.pth"), map_location="cpu", weights_only=False)      # this process stays off the GPU
    assert sorted(latest) == ["best_val_loss", "epoch", "global_step", "iter", "net_state_dict", "optimizer_state_dict", "seed",
                              "world_size"]
    assert (latest["epoch"], latest["global_step"], latest["seed"], latest["world_size"]) == (2, 4, 5, 2)

    # 5, 6
    for r in (0, 1):
        o, a, c = res[r], res[r]["A"], res[r]["C"]
        assert (c["world"], c["rank"]) == (1, 0)
        for k in ("global_step", "epoch", "lr", "last_sched", "steps"):
            assert a[k] == c[k], k
        assert c["files"] == ["_renderer", "best.pth", "epoch_0000.pth", "epoch_0001.pth", "latest.pth"]
        val_w, val_1 = o["val"]
        print(f"rank {r}: after 2 epochs, validation loss under 2 ranks {val_w:.9g}, under 1 rank {val_1:.9g} (relative difference "
              f"{abs(val_w - val_1) / abs(val_1):.3e}); trajectory distance |p_2 - p_1| / |p_1 - p_init| = {o['distance']:.3e}, "
              f"max |p_2 - p_1| = {o['max_param_diff']:.3e}  [the distance is reported, not bounded: Adam's first steps are "
              "sign-sensitive where a gradient is near zero]")
        assert abs(val_w - val_1) <= LOSS_RTOL * abs(val_1)
        assert o["D_loaded"] == (2, 4, True, a["last_sched"])
        assert o["D_done"] == (6, 6, True, True, False)
    assert res[0]["val"][0] == res[1]["val"][0]                                             # one collective, one value
    assert not torch.cuda.is_initialized()
