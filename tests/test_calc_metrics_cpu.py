"""calc_metrics, host side: the two entry points are declared and exported, every argument check of pnr_eval_frames_u8 (all
made before any launch, so they run without a GPU), the workspace size, the reduce step against the reference's own
all_metrics.txt (tests/golden/calc_metrics_reduce.npz, tools/gen_golden_calc_metrics.py), the map step with metrics="host" on
trees written into tmp_path — which views count, the list filter, resume, the text of metrics.txt, what is refused, the LPIPS
hook — and two gloo ranks against one process."""
import os
import re
import shutil
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_WORKSPACE = -1, -2, -4
H, W = 9, 11


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_both_prototypes_are_declared_bound_and_exported():
    from pixel_nerf_multiscale_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "pnr.h")).read()
    declared = set(re.findall(r"\b(pnr_[a-z0-9_]+)\s*\(", hdr))
    for name in ("pnr_eval_frames_u8", "pnr_eval_frames_u8_workspace_bytes"):
        assert name in declared and name in N.PROTOTYPES and hasattr(N.lib, name), name


def test_eval_frames_u8_checks_arguments_without_gpu():
    from pixel_nerf_multiscale_amd import _native as N
    L = N.lib
    p = 64          # a non-NULL value: the checks below return before anything dereferences or launches
    big = 1 << 40

    def ef(pred=p, pc=3, gt=p, gc=3, F=2, W=16, H=16, pp=None, gp=None, m=p, ws=p, ws_bytes=big):
        return L.pnr_eval_frames_u8(pred, pc, gt, gc, F, W, H, pp, gp, m, ws, ws_bytes, None)

    for name in ("pred", "gt", "m", "ws"):
        assert ef(**{name: None}) == E_NULL, name
    assert ef(F=0) == E_SHAPE and ef(F=-1) == E_SHAPE
    for w, h in ((6, 16), (16, 6), (6, 6), (0, 16), (16, -1)):      # below the 7 x 7 window
        assert ef(W=w, H=h) == E_SHAPE
    for ch in (0, 1, 2, 5, -3):
        assert ef(pc=ch) == E_SHAPE and ef(gc=ch) == E_SHAPE and ef(pc=ch, gc=4) == E_SHAPE
    assert ef(F=1, W=65536, H=32768) == E_SHAPE                     # W * H = 2^31
    assert ef(F=1, W=46341, H=46341) == E_SHAPE                     # just above 2^31
    assert ef(F=(1 << 23) + 1) == E_SHAPE                           # F x tiles above 2^23 workgroups
    assert ef(F=(1 << 15) + 1, W=256, H=256) == E_SHAPE             # 256 tiles per frame
    assert ef(F=3, W=32768, H=32768) == E_SHAPE                     # 2^22 tiles per frame: two frames are the limit
    need = L.pnr_eval_frames_u8_workspace_bytes(2, 16, 16)
    assert need > 0 and ef(ws_bytes=need - 1) == E_WORKSPACE and ef(ws_bytes=0) == E_WORKSPACE
    assert ef(pc=4, gc=4, pp=p, gp=p, ws_bytes=need - 1) == E_WORKSPACE
    assert ef(F=3, W=300, H=400, ws_bytes=L.pnr_eval_frames_u8_workspace_bytes(2, 300, 400)) == E_WORKSPACE
    with pytest.raises(ValueError):
        N.check(ef(ws_bytes=0), "pnr_eval_frames_u8")


def test_workspace_is_that_of_eval_frames():
    from pixel_nerf_multiscale_amd import _native as N
    wb, wb_f32 = N.lib.pnr_eval_frames_u8_workspace_bytes, N.lib.pnr_eval_frames_workspace_bytes
    for F, w, h in ((1, 7, 7), (3, 16, 16), (3, 17, 16), (2, 23, 37), (250, 128, 128), (49, 400, 300), (1 << 15, 256, 256)):
        tiles = ((w + 15) // 16) * ((h + 15) // 16)
        assert wb(F, w, h) == wb_f32(F, w, h) == F * tiles * 16, (F, w, h)
    for F, w, h in ((0, 16, 16), (-2, 16, 16), (1, 6, 16), (1, 16, 6), (1, 0, 16), (1, 65536, 32768), ((1 << 15) + 1, 256, 256),
                    ((1 << 23) + 1, 7, 7)):
        assert wb(F, w, h) == 0, (F, w, h)


def test_eval_frames_u8_wrapper_checks_shapes_on_the_host():
    from pixel_nerf_multiscale_amd import util
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    for pred, gt in ((u8(2, 8, 8, 3).float(), u8(2, 8, 8, 3)),          # not bytes
                     (u8(2, 8, 8, 3), u8(2, 3, 8, 8)),                  # planar
                     (u8(2, 8, 8, 2), u8(2, 8, 8, 3)),                  # two channels
                     (u8(3, 8, 8, 3), u8(2, 8, 8, 4)),                  # another number of frames
                     (u8(2, 8, 8, 3), u8(2, 8, 9, 3)),                  # another size
                     (u8(8, 8, 3), u8(8, 8, 3)),                        # no frame axis
                     (u8(0, 8, 8, 3), u8(0, 8, 8, 3))):                 # no frame
        with pytest.raises(ValueError):
            util.eval_frames_u8(pred, gt)


# ------------------------------------------------------------------------------------------------------------- the reduce
@pytest.mark.parametrize("case", ["plain", "multicat", "dtu_sort"])
def test_reduce_writes_the_references_bytes(case, tmp_path):
    from pixel_nerf_multiscale_amd import evalio
    g = np.load(os.path.join(ROOT, "tests", "golden", "calc_metrics_reduce.npz"))
    assert sorted(g["cases"].tolist()) == ["dtu_sort", "multicat", "plain"]
    datadir, output = tmp_path / "data", tmp_path / "render"
    datadir.mkdir()
    output.mkdir()
    objects, texts, metadata = g[f"{case}__objects"].tolist(), g[f"{case}__metrics"].tolist(), str(g[f"{case}__metadata"])
    assert (metadata != "") == (case == "multicat")
    if metadata:
        (datadir / "metadata.yaml").write_text(metadata)
    for obj, text in zip(objects, texts):
        (output / obj).mkdir()
        if not obj.startswith("_"):
            (output / obj / "metrics.txt").write_text(text)
    (output / "finish.txt").write_text("x 1.0 1.0 1\n")
    want = g[f"{case}__all_metrics"].tobytes()
    totals = evalio.metrics_reduce(str(datadir), str(output), multicat=case == "multicat", dtu_sort=case == "dtu_sort", verbose=False)
    assert (output / "all_metrics.txt").read_bytes() == want
    assert totals.text.encode() == want
    last = want.decode().splitlines()[-1]
    for name in ("psnr", "ssim", "lpips"):
        assert "{}: {:.6f}".format(name, totals[name]) in last
    # the same through calc_metrics(reduce_only=True)
    os.remove(output / "all_metrics.txt")
    again = evalio.calc_metrics(str(datadir), str(output), reduce_only=True, multicat=case == "multicat",
                                dtu_sort=case == "dtu_sort", verbose=False)
    assert (output / "all_metrics.txt").read_bytes() == want and dict(again) == dict(totals)
    if case == "multicat":
        assert len(want.decode().splitlines()) == 3 + 2 and "03001627.psnr" in totals and "02958343.psnr" in totals
    if case == "dtu_sort":                                          # the lexical order cannot even be the numeric one
        assert sorted(objects) != sorted(objects, key=lambda x: int(x[4:]))


def test_reduce_refuses_files_that_disagree_about_the_names(tmp_path):
    from pixel_nerf_multiscale_amd import evalio
    for obj, text in (("a", "psnr 20.0\nssim 0.5"), ("b", "psnr 21.0\nssim 0.6\nlpips 0.1")):
        (tmp_path / obj).mkdir()
        (tmp_path / obj / "metrics.txt").write_text(text)
    with pytest.raises(ValueError, match="b/metrics.txt"):
        evalio.metrics_reduce(str(tmp_path), str(tmp_path), verbose=False)
    (tmp_path / "b" / "metrics.txt").write_text("psnr 21.0\nssim 0.625")
    totals = evalio.metrics_reduce(str(tmp_path), str(tmp_path), verbose=False)
    assert totals.text == " psnr: 20.500000 ssim: 0.562500" and dict(totals) == {"psnr": 20.5, "ssim": 0.5625}
    (tmp_path / "b" / "metrics.txt").write_text("psnr 21.0\nmse 0.625")
    with pytest.raises(ValueError):
        evalio.metrics_reduce(str(tmp_path), str(tmp_path), verbose=False)
    with pytest.raises(ValueError):
        evalio.metrics_reduce(str(tmp_path), str(tmp_path / "a"), verbose=False)      # no object folder


# ---------------------------------------------------------------------------------------------------------------- the map
def _images(obj_seed, n_views, h=H, w=W):
    """-> [(gt (h, w, 3) uint8, render (h, w, 3) uint8)] per view: seeded noise, the render a few levels off."""
    rng = np.random.default_rng(obj_seed)
    out = []
    for _ in range(n_views):
        gt = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        pred = np.clip(gt.astype(np.int64) + rng.integers(-20, 21, gt.shape), 0, 255).astype(np.uint8)
        out.append((gt, pred))
    return out


def _save(path, a):
    from PIL import Image
    Image.fromarray(a).save(path, **({"quality": 95} if str(path).endswith(".jpg") else {}))


def _load(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im, dtype=np.uint8)


def _write_object(evalio, im_root, rend, views, gt_kind=None, gt_name="{:06}"):
    """views: {view index: (gt, render)}; gt_kind: {view: "rgba" | "jpg"}.  -> {view: (gt file, render file)}."""
    os.makedirs(im_root)
    os.makedirs(rend)
    files = {}
    for v, (gt, pred) in views.items():
        kind = (gt_kind or {}).get(v, "png")
        gt_path = os.path.join(im_root, gt_name.format(v) + (".jpg" if kind == "jpg" else ".png"))
        if kind == "png":
            evalio.write_png(gt_path, gt)
        elif kind == "rgba":
            alpha = np.random.default_rng(v).integers(0, 256, gt.shape[:2] + (1,), dtype=np.uint8)
            _save(gt_path, np.concatenate([gt, alpha], -1))
        else:
            _save(gt_path, gt)
        rend_path = os.path.join(rend, "{:06}.png".format(v))
        evalio.write_png(rend_path, pred)
        files[v] = (gt_path, rend_path)
    return files


def _expected(evalio, files, views):
    """The per-object means over `views` by the host functions on the files' bytes, and the text of metrics.txt."""
    ps = ss = 0.0
    for v in views:
        gt = _load(files[v][0]).astype(np.float32)[..., :3] / 255.0
        pred = _load(files[v][1]).astype(np.float32) / 255.0
        ps += float(evalio.psnr(pred, gt))
        ss += evalio.ssim(pred, gt)
    return ps / len(views), ss / len(views), "psnr {}\nssim {}".format(ps / len(views), ss / len(views))


def _srn_tree(evalio, root, objs=("o1", "o2"), n_views=6, gt_kind=None):
    """datadir/<obj>/rgb/<view:06>.png|jpg and render/<obj>/<view:06>.png -> (datadir, output, {obj: files})."""
    datadir, output = os.path.join(root, "data"), os.path.join(root, "render")
    files = {}
    for k, obj in enumerate(objs):
        views = dict(enumerate(_images(11 + k, n_views)))
        files[obj] = _write_object(evalio, os.path.join(datadir, obj, "rgb"), os.path.join(output, obj), views, gt_kind)
    return datadir, output, files


def _metrics_txt(output, obj):
    return open(os.path.join(output, obj, "metrics.txt")).read()


def test_map_writes_the_host_functions_numbers(tmp_path):
    from pixel_nerf_multiscale_amd import evalio
    datadir, output, files = _srn_tree(evalio, str(tmp_path), gt_kind={1: "rgba", 4: "jpg"})
    assert _load(files["o1"][1][0]).shape == (H, W, 4) and files["o1"][4][0].endswith(".jpg")
    open(os.path.join(datadir, "o1", "rgb", "notes.txt"), "w").write("not an image")
    written = evalio.metrics_map(datadir, output, dataset_format="srn", verbose=False)
    assert sorted(written) == [os.path.join(output, o, "metrics.txt") for o in ("o1", "o2")]
    for obj in ("o1", "o2"):
        assert _metrics_txt(output, obj) == _expected(evalio, files[obj], range(6))[2]
    # the RGBA view counts with its first three channels: the same numbers as the plain file
    p_rgba = _expected(evalio, files["o1"], [1])[0]
    gt, pred = _images(11, 6)[1]
    assert p_rgba == float(evalio.psnr(pred.astype(np.float32) / 255.0, gt.astype(np.float32) / 255.0))
    totals = evalio.metrics_reduce(datadir, output, verbose=False)
    want = [_expected(evalio, files[o], range(6)) for o in ("o1", "o2")]
    mean = lambda k: (float(str(want[0][k])) + float(str(want[1][k]))) / 2
    assert totals.text == " psnr: {:.6f} ssim: {:.6f}".format(mean(0), mean(1))


def test_map_counts_the_references_views(tmp_path):
    from pixel_nerf_multiscale_amd import evalio
    datadir, output, files = _srn_tree(evalio, str(tmp_path), objs=("o1",), n_views=8)
    os.remove(files["o1"][7][1])                                    # a ground-truth view that was never rendered
    os.remove(files["o1"][6][0])                                    # a render without ground truth
    evl = tmp_path / "eval_views.txt"
    evl.write_text("0 2 3 5 7\n9 9 9\n")                            # the first line counts
    cases = [(dict(), [0, 1, 2, 3, 4, 5]),
             (dict(primary="0 2"), [1, 3, 4, 5]),
             (dict(primary=[5]), [0, 1, 2, 3, 4]),
             (dict(exclude_dtu_bad=True), [0, 1, 2]),
             (dict(exclude_dtu_bad=True, primary="1"), [0, 2]),
             (dict(eval_view_list=str(evl)), [0, 2, 3, 5]),
             (dict(eval_view_list=[1, 4, 6]), [1, 4]),
             (dict(eval_view_list=str(evl), primary="0", exclude_dtu_bad=True), [2])]
    for kw, views in cases:
        evalio.metrics_map(datadir, output, dataset_format="srn", overwrite=True, verbose=False, **kw)
        assert _metrics_txt(output, "o1") == _expected(evalio, files["o1"], views)[2], kw
    with pytest.raises(ValueError, match="o1"):                     # nothing left to count
        evalio.metrics_map(datadir, output, dataset_format="srn", overwrite=True, verbose=False, eval_view_list=[6, 7])


def _dvr_tree(evalio, root, cats):
    """cats: {cat: [obj]}, "." for a tree without categories.  datadir/<cat>/<obj>/image/<view:04>.png, a softras_test.lst per
    category folder, render/<cat>_<obj> -> (datadir, output, {render name: files})."""
    datadir, output = os.path.join(root, "data"), os.path.join(root, "render")
    files, k = {}, 0
    for cat, objs in cats.items():
        for obj in objs:
            name = obj if cat == "." else cat + "_" + obj
            views = dict(enumerate(_images(31 + k, 4)))
            files[name] = _write_object(evalio, os.path.join(datadir, cat, obj, "image"), os.path.join(output, name), views,
                                        gt_name="{:04}")
            k += 1
    return datadir, output, files


def test_map_filters_by_the_list_file_and_the_render_folders(tmp_path):
    from pixel_nerf_multiscale_amd import evalio
    datadir, output, files = _dvr_tree(evalio, str(tmp_path), {".": ["aa", "bb", "cc", "dd"]})
    open(os.path.join(datadir, "softras_test.lst"), "w").write("aa\ncc\ndd\nzz\n")
    open(os.path.join(datadir, "other.lst"), "w").write("bb\n")
    shutil.rmtree(os.path.join(output, "dd"))                       # listed, never rendered: not AVAILABLE
    written = evalio.metrics_map(datadir, output, verbose=False)    # dataset_format="dvr", list_name="softras_test"
    assert sorted(os.path.basename(os.path.dirname(p)) for p in written) == ["aa", "cc"]
    assert not os.path.exists(os.path.join(output, "bb", "metrics.txt")) and not os.path.exists(os.path.join(output, "dd"))
    assert _metrics_txt(output, "aa") == _expected(evalio, files["aa"], range(4))[2]      # "0002.png" against "000002.png"
    written = evalio.metrics_map(datadir, output, list_name="other", verbose=False)
    assert [os.path.basename(os.path.dirname(p)) for p in written] == ["bb"]
    with pytest.raises(NotImplementedError):
        evalio.metrics_map(datadir, output, dataset_format="llff", verbose=False)
    with pytest.raises(ValueError, match="metrics"):
        evalio.metrics_map(datadir, output, metrics="gpu", verbose=False)


def test_map_skips_an_existing_metrics_file_unless_overwrite(tmp_path):
    from pixel_nerf_multiscale_amd import evalio
    datadir, output, files = _srn_tree(evalio, str(tmp_path))
    open(os.path.join(output, "o1", "metrics.txt"), "w").write("psnr 1.0\nssim 1.0")
    written = evalio.metrics_map(datadir, output, dataset_format="srn", verbose=False)
    assert written == [os.path.join(output, "o2", "metrics.txt")]
    assert _metrics_txt(output, "o1") == "psnr 1.0\nssim 1.0"
    assert evalio.metrics_map(datadir, output, dataset_format="srn", verbose=False) == []
    written = evalio.metrics_map(datadir, output, dataset_format="srn", overwrite=True, verbose=False)
    assert len(written) == 2 and _metrics_txt(output, "o1") == _expected(evalio, files["o1"], range(6))[2]


def test_multicat_names_viewlist_and_the_category_table(tmp_path):
    import json
    from pixel_nerf_multiscale_amd import evalio
    cats = {"02691156": ["p1", "p2"], "03001627": ["c1"]}
    datadir, output, files = _dvr_tree(evalio, str(tmp_path), cats)
    for cat, objs in cats.items():
        open(os.path.join(datadir, cat, "softras_test.lst"), "w").write("\n".join(objs))
    meta = {"02691156": {"name": "airplane,aeroplane"}, "03001627": {"name": "chair"}, "04530566": {"name": "vessel,ship"}}
    json.dump(meta, open(os.path.join(datadir, "metadata.yaml"), "w"))      # a FILE among the category folders
    lut = tmp_path / "src_dvr.txt"
    lut.write_text("02691156 p1 0\n02691156 p2 1 3\n03001627 c1 2\n")
    counted = {"02691156_p1": [1, 2], "02691156_p2": [0, 2], "03001627_c1": [0, 1]}      # minus the table's views and view 3
    totals = evalio.calc_metrics(datadir, output, multicat=True, viewlist=str(lut), primary="3", verbose=False)
    want = {name: _expected(evalio, files[name], views) for name, views in counted.items()}
    for name in counted:
        assert _metrics_txt(output, name) == want[name][2], name
    r = lambda name, k: float(str(want[name][k]))                   # what the reduce reads back from the text
    plane = [(r("02691156_p1", k) + r("02691156_p2", k)) / 2 for k in (0, 1)]
    chair = [r("03001627_c1", k) for k in (0, 1)]
    total = [(r("02691156_p1", k) + r("02691156_p2", k) + r("03001627_c1", k)) / 3 for k in (0, 1)]
    text = ("{:12s} psnr: {:.6f} ssim: {:.6f} n_inst: 2\n".format("airplane", *plane)
            + "{:12s} psnr: {:.6f} ssim: {:.6f} n_inst: 1\n".format("chair", *chair)
            + "---\n{:12s} psnr: {:.6f} ssim: {:.6f}".format("total", *total))
    assert open(os.path.join(output, "all_metrics.txt")).read() == text == totals.text
    assert totals["psnr"] == total[0] and totals["03001627.ssim"] == chair[1]
    # the table as a dict, as evalio.read_source_view_lut gives it; an object it does not list is refused by name
    table = evalio.read_source_view_lut(str(lut))
    evalio.metrics_map(datadir, output, multicat=True, viewlist=table, primary="3", overwrite=True, verbose=False)
    assert _metrics_txt(output, "02691156_p2") == want["02691156_p2"][2]
    del table["03001627/c1"]
    with pytest.raises(ValueError, match="03001627_c1"):
        evalio.metrics_map(datadir, output, multicat=True, viewlist=table, overwrite=True, verbose=False)


def test_map_refuses_what_it_cannot_compare(tmp_path):
    from pixel_nerf_multiscale_amd import evalio

    def tree(sub):
        return _srn_tree(evalio, str(tmp_path / sub), objs=("o1",), n_views=3)

    def run(datadir, output):
        return evalio.metrics_map(datadir, output, dataset_format="srn", verbose=False)

    datadir, output, files = tree("grey_render")
    _save(files["o1"][1][1], _images(1, 1)[0][0][..., 0])           # mode L
    with pytest.raises(ValueError, match="000001.png"):
        run(datadir, output)
    datadir, output, files = tree("rgba_render")
    _save(files["o1"][2][1], np.concatenate([_images(1, 1)[0][0], np.full((H, W, 1), 255, np.uint8)], -1))
    with pytest.raises(ValueError, match="render.o1.000002.png"):
        run(datadir, output)
    datadir, output, files = tree("grey_gt")
    _save(files["o1"][0][0], _images(1, 1)[0][0][..., 0])
    with pytest.raises(ValueError, match="rgb.000000.png"):
        run(datadir, output)
    datadir, output, files = tree("sixteen_bit_gt")
    _save(files["o1"][0][0], np.arange(H * W, dtype=np.uint16).reshape(H, W) * 300)      # mode I;16
    with pytest.raises(ValueError, match="rgb.000000.png"):
        run(datadir, output)
    datadir, output, files = tree("pair_of_two_sizes")
    evalio.write_png(files["o1"][1][1], _images(1, 1, H, W + 1)[0][1])
    with pytest.raises(ValueError, match="o1"):
        run(datadir, output)
    datadir, output, files = tree("object_of_two_sizes")
    gt, pred = _images(1, 1, H + 2, W)[0]
    evalio.write_png(files["o1"][2][0], gt)
    evalio.write_png(files["o1"][2][1], pred)
    with pytest.raises(ValueError, match="o1.*two sizes"):
        run(datadir, output)
    datadir, output, files = tree("no_view")
    for v in range(3):
        os.remove(files["o1"][v][1])
    with pytest.raises(ValueError, match="o1"):
        run(datadir, output)
    assert not os.path.exists(os.path.join(output, "o1", "metrics.txt"))


def test_lpips_hook_sees_batches_in_range_and_its_mean_is_written(tmp_path):
    from pixel_nerf_multiscale_amd import evalio
    datadir, output, files = _srn_tree(evalio, str(tmp_path), objs=("o1",), n_views=7, gt_kind={2: "rgba"})
    calls = []

    def stub(pred, gt):
        assert pred.dtype == torch.float32 and gt.dtype == torch.float32 and pred.shape == gt.shape
        assert tuple(pred.shape[1:]) == (3, H, W) and not pred.requires_grad
        assert float(pred.min()) >= -1.0 and float(pred.max()) <= 1.0 and float(gt.min()) >= -1.0 and float(gt.max()) <= 1.0
        calls.append((pred.clone(), gt.clone()))
        return (pred - gt).abs().mean(dim=(1, 2, 3), keepdim=True)      # (n, 1, 1, 1), as the lpips package returns

    evalio.metrics_map(datadir, output, dataset_format="srn", lpips=stub, lpips_batch_size=3, verbose=False)
    assert [c[0].shape[0] for c in calls] == [3, 3, 1]
    preds, gts = torch.cat([c[0] for c in calls]), torch.cat([c[1] for c in calls])
    for v in range(7):                                              # in view order, the values of calc_metrics.py:232-233
        gt = _load(files["o1"][v][0]).astype(np.float32)[..., :3] / 255.0
        pred = _load(files["o1"][v][1]).astype(np.float32) / 255.0
        assert np.array_equal(gts[v].numpy(), (gt * np.float32(2) - np.float32(1)).transpose(2, 0, 1))
        assert np.array_equal(preds[v].numpy(), (pred * np.float32(2) - np.float32(1)).transpose(2, 0, 1))
    want = torch.cat([stub(p, g).reshape(-1).double() for p, g in list(calls)]).mean().item()
    assert _metrics_txt(output, "o1") == _expected(evalio, files["o1"], range(7))[2] + "\nlpips {}".format(want)
    totals = evalio.metrics_reduce(datadir, output, verbose=False)
    assert list(totals) == ["psnr", "ssim", "lpips"] and totals.text.endswith(" lpips: {:.6f}".format(want))


# ------------------------------------------------------------------------------------------------------------- two ranks
def _rank(rank, world, port, datadir, output, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pixel_nerf_multiscale_amd import evalio
        totals = evalio.calc_metrics(datadir, output, dataset_format="srn", metrics="host", verbose=False)
        q.put((rank, dict(totals), totals.text))
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_write_what_one_process_writes(tmp_path):
    from pixel_nerf_multiscale_amd import evalio
    objs = ("o1", "o2", "o3")
    datadir, output, _ = _srn_tree(evalio, str(tmp_path), objs=objs, n_views=3)
    output2 = os.path.join(str(tmp_path), "render_two_ranks")
    shutil.copytree(output, output2)
    single = evalio.calc_metrics(datadir, output, dataset_format="srn", metrics="host", verbose=False)

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, datadir, output2, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == [0, 1]
    for _, totals, text in res:                                     # every rank returns rank 0's totals
        assert totals == dict(single) and text == single.text
    for name in [os.path.join(o, "metrics.txt") for o in objs] + ["all_metrics.txt"]:
        assert open(os.path.join(output2, name), "rb").read() == open(os.path.join(output, name), "rb").read(), name
    assert sorted(os.listdir(output2)) == sorted(os.listdir(output))
