"""The training loop without a GPU: the checkpoint rotation as a pure function, the helpers that make a run reproducible
(the epoch's permutation, the source-view count of a keyed step) and the refusals Trainer makes before it touches a device."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pixel_nerf_multiscale_amd.parallel import frame_seed


def _names(epochs):
    return ["epoch_%04d.pth" % e for e in epochs]


OTHERS = ["latest.pth", "best.pth", "_renderer", "epoch_.pth", "epoch_12.pth.tmp", "myepoch_0003.pth", "epoch_0003.pt", "notes.txt"]


# ------------------------------------------------------------------------------------------------------------ rotation
def test_keep_last_keeps_the_lexicographically_last():
    from pixel_nerf_multiscale_amd.trainer import checkpoints_to_remove
    names = _names([3, 0, 2, 1, 4]) + OTHERS
    assert checkpoints_to_remove(names, "keep_last", 2, 4) == _names([0, 1, 2])
    assert checkpoints_to_remove(names, "keep_last", 5, 4) == [] and checkpoints_to_remove(names, "keep_last", 20, 4) == []
    assert checkpoints_to_remove(names, "keep_last", 1, 4) == _names([0, 1, 2, 3])
    assert checkpoints_to_remove(OTHERS, "keep_last", 0, 0) == []                       # foreign names are never candidates
    # lexicographic, as the reference's sorted(glob): a five-digit epoch sorts in front of epoch_9999
    assert checkpoints_to_remove(["epoch_9999.pth", "epoch_10000.pth"], "keep_last", 1, 10000) == ["epoch_10000.pth"]


def test_keep_all_keeps_everything():
    from pixel_nerf_multiscale_amd.trainer import checkpoints_to_remove
    assert checkpoints_to_remove(_names(range(300)) + OTHERS, "keep_all", 1, 299) == []


def test_milestone_boundaries():
    from pixel_nerf_multiscale_amd.trainer import checkpoints_to_remove
    names = _names(range(0, 131)) + OTHERS
    gone = checkpoints_to_remove(names, "milestone", 20, 123)
    kept = sorted(set(_names(range(0, 131))) - set(gone))
    want = list(range(0, 11)) + list(range(15, 101, 5)) + [120, 123]
    assert kept == _names(want)
    assert not set(gone) & set(OTHERS)
    # the edges one by one: 10 stays and 11 goes, 100 stays, 105 goes (past 100 only multiples of 20 stay), 120 stays
    for e, stays in ((10, True), (11, False), (100, True), (105, False), (120, True), (110, False), (140, True), (95, True), (96, False)):
        assert (checkpoints_to_remove(_names([e]), "milestone", 20, 500) == []) is stays, e
    assert checkpoints_to_remove(_names([11]), "milestone", 20, 11) == []               # the current epoch always stays
    assert checkpoints_to_remove(_names([105]), "milestone", 20, 105) == []


def test_unknown_strategy_is_refused():
    from pixel_nerf_multiscale_amd.trainer import checkpoints_to_remove
    with pytest.raises(ValueError, match="save_strategy"):
        checkpoints_to_remove([], "newest", 1, 0)


# ------------------------------------------------------------------------------------------------------------ determinism
def test_epoch_permutation_depends_on_seed_and_epoch_only():
    from pixel_nerf_multiscale_amd.trainer import epoch_permutation
    torch.manual_seed(1)
    a = epoch_permutation(50, 7, 3)
    torch.manual_seed(2)
    torch.rand(5)
    b = epoch_permutation(50, 7, 3)
    assert torch.equal(a, b) and sorted(a.tolist()) == list(range(50))
    assert torch.equal(a, torch.randperm(50, generator=torch.Generator().manual_seed(frame_seed(7, 3))))
    assert not torch.equal(a, epoch_permutation(50, 7, 4)) and not torch.equal(a, epoch_permutation(50, 8, 3))
    state = torch.get_rng_state()
    epoch_permutation(50, 7, 5)
    assert torch.equal(state, torch.get_rng_state())                                   # the global generator is not consumed


def test_trainer_is_reexported_and_curr_nviews_follows_the_key():
    from pixel_nerf_multiscale_amd import train, trainer
    assert train.Trainer is trainer.Trainer
    nviews = [1, 2, 3]
    for step in range(6):
        key = frame_seed(11, step)
        assert train.curr_nviews_for(nviews, key) == nviews[key % 3]
    assert {train.curr_nviews_for(nviews, frame_seed(11, s)) for s in range(40)} == {1, 2, 3}


# ------------------------------------------------------------------------------------------------------------ refusals
class _Data(list):
    z_near, z_far = 0.8, 1.8


def _kw(tmp_path, **more):
    return dict(name="run", checkpoints_path=str(tmp_path / "ckpt"), logs_path=str(tmp_path / "logs"), batch_size=2, ray_batch_size=8,
                nviews=[1], loss=None, **more)


def test_refusals_come_before_any_device_work(tmp_path):
    from pixel_nerf_multiscale_amd.trainer import Trainer
    net = torch.nn.Linear(2, 2)
    with pytest.raises(FileNotFoundError):
        Trainer(net, None, _Data(), None, **_kw(tmp_path, resume=str(tmp_path / "nowhere" / "epoch_0007.pth")))
    with pytest.raises(ValueError, match="lr_policy"):
        Trainer(net, None, _Data(), None, **_kw(tmp_path, lr_policy="cosine"))
    with pytest.raises(ValueError, match="save_strategy"):
        Trainer(net, None, _Data(), None, **_kw(tmp_path, save_strategy="newest"))
    with pytest.raises(ValueError, match="draws"):
        Trainer(net, None, _Data(), None, **_kw(tmp_path, draws="gpu"))
    assert not os.path.exists(tmp_path / "ckpt")                                        # nothing was created on the way


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, root, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pixel_nerf_multiscale_amd.trainer import Trainer
        try:
            Trainer(torch.nn.Linear(2, 2), None, _Data(), None, name="run", checkpoints_path=root, logs_path=root, batch_size=2,
                    ray_batch_size=8, nviews=[1], loss=None)
            q.put((rank, "no error"))
        except NotImplementedError as e:
            q.put((rank, str(e)))
    finally:
        dist.destroy_process_group()


def test_a_process_group_of_two_ranks_is_refused(tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r for r, _ in res) == [0, 1]
    for _, msg in res:
        assert "parallel.allreduce_gradients" in msg and "2 ranks" in msg
