"""Training back end on the device: pnr_adam_step through optim.DeviceAdam, and train.train_step on top.

The yardstick is the fp64 model of include/pnr.h's arithmetic (optim_util.AdamModel).  No tolerance is fixed here: wherever
p, m, v are compared, the kernel's worst |x - model| may be at most 2x the worst error of torch's own fp32 Adam
(torch.optim.Adam(foreach=False) + clip_grad_norm_, on the CPU) against the model IN THE SAME CASE — both are correctly
rounded fp32 sequences in different orders (lerp against multiply-add) and the last rounding of p dominates both.
grad_norm: relative error against the exactly summed fp64 norm at most (longest addition path + 2) * 2^-53, the kernel's
path being 16 (a thread's elements) + 8 (its workgroup's tree) + ceil(n_chunks / 256) + 8 (the one-workgroup pass).
Every test prints what it measured (-s)."""
import math

import numpy as np
import pytest
import torch

import optim_util as ou
from eval_util import sync_debug_mode_works

pytestmark = pytest.mark.gpu

LR, BETAS, EPS, MAX_NORM = ou.LR, ou.BETAS, ou.EPS, ou.MAX_NORM


def _chunk():
    from pixel_nerf_multiscale_amd import _native as N
    return int(N.lib.pnr_optim_chunk_elems())


CHUNK = _chunk()                 # the library's chunk size: the edge sizes and the path-length bound follow it


def _device_adam(params, **kw):
    """-> (cuda parameters, DeviceAdam) over fp32 copies of `params`."""
    from pixel_nerf_multiscale_amd.optim import DeviceAdam
    tp = [torch.nn.Parameter(torch.from_numpy(np.asarray(p, dtype=np.float32).copy()).cuda()) for p in params]
    kw.setdefault("lr", LR)
    kw.setdefault("max_norm", MAX_NORM)
    return tp, DeviceAdam(tp, betas=BETAS, eps=EPS, **kw)


def _set_grads(tp, opt, G):
    """Gradients as backward leaves them: written into the .grad the optimizer owns (None: no gradient this step)."""
    for i, (t, g) in enumerate(zip(tp, G)):
        if g is None:
            t.grad = None
        else:
            if t.grad is None:
                t.grad = opt._slices[i]
            t.grad.copy_(torch.from_numpy(np.asarray(g, dtype=np.float32)).view_as(t))


def _state(tp, opt):
    p = [t.detach().cpu().numpy() for t in tp]
    m = [opt.moments(i)[0].cpu().numpy() for i in range(len(tp))]
    v = [opt.moments(i)[1].cpu().numpy() for i in range(len(tp))]
    return p, m, v


def _bits(arrs):
    return [np.ascontiguousarray(a).view(np.int32).copy() for a in arrs]


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


def _adam_state_dict(m, v, step, lr=LR):
    """torch.optim.Adam's state_dict format from numpy moments."""
    return {"state": {i: {"step": torch.tensor(float(step)), "exp_avg": torch.from_numpy(np.asarray(a, dtype=np.float32).copy()),
                          "exp_avg_sq": torch.from_numpy(np.asarray(b, dtype=np.float32).copy())} for i, (a, b) in enumerate(zip(m, v))},
            "param_groups": [{"lr": lr, "betas": BETAS, "eps": EPS, "weight_decay": 0, "amsgrad": False, "maximize": False,
                              "foreach": False, "capturable": False, "differentiable": False, "fused": None,
                              "params": list(range(len(m)))}]}


def _compare(what, kernel, torch_, model):
    """kernel / torch_ / model: (p, m, v).  Prints both errors per quantity and holds the kernel to 2x torch's."""
    for q, k, t, r in zip("pmv", kernel, torch_, model):
        ek, et = ou.worst(k, r), ou.worst(t, r)
        print(f"{what}: max |{q} - model|  kernel {ek:.3e}  torch fp32 {et:.3e}  ratio {ek / et if et else float('nan'):.2f}")
        assert ek <= 2.0 * et, (what, q, ek, et)


# ------------------------------------------------------------------------------------------------- one step, trajectory
def test_one_step_from_a_shared_state():
    """p, m, v of the trajectory after 10 steps, rounded to fp32, are the state all three start from (t = 10)."""
    params, grads, err, snaps = ou.torch_reference()
    s = snaps[9]
    p0, m0, v0 = ([a.astype(np.float32) for a in s[k]] for k in "pmv")
    G = grads[10]
    model = ou.AdamModel(p0, LR, BETAS, EPS, MAX_NORM)
    model.m, model.v, model.t = [a.astype(np.float64) for a in m0], [a.astype(np.float64) for a in v0], 10
    model.step(G)
    ttp, topt, tstep = ou.torch_adam_cpu(p0, m0, v0, step=10)
    tstep(G)
    tp, opt = _device_adam(p0)
    opt.load_state_dict(_adam_state_dict(m0, v0, 10))
    _set_grads(tp, opt, G)
    opt.step()
    assert int(opt.step_count) == 11 and int(opt.found_inf) == 0 and int(opt.skipped) == 0
    assert float(opt.clip_coef) == float(model.clip_coef)
    _compare("one step", _state(tp, opt), ou.torch_state(ttp, topt), (model.p, model.m, model.v))


def test_trajectory_of_40_steps():
    params, grads, err, snaps = ou.torch_reference()
    tp, opt = _device_adam(params)
    worst_ratio = {q: 0.0 for q in "pmv"}
    for k, G in enumerate(grads):
        _set_grads(tp, opt, G)
        opt.step()
        got = _state(tp, opt)
        for q, a in zip("pmv", got):
            ek = ou.worst(a, snaps[k][q])
            worst_ratio[q] = max(worst_ratio[q], ek / err[k][q])
            assert ek <= 2.0 * err[k][q], (k + 1, q, ek, err[k][q])          # the bound holds after EVERY step
            if k + 1 in (1, 2, 10, ou.STEPS):
                print(f"step {k + 1}: max |{q} - model|  kernel {ek:.3e}  torch fp32 {err[k][q]:.3e}  ratio {ek / err[k][q]:.2f}")
        assert float(opt.clip_coef) == float(snaps[k]["clip_coef"]), k
    print("worst kernel / torch error ratio over the 40 steps: " + "  ".join(f"{q} {r:.2f}" for q, r in worst_ratio.items()))
    assert int(opt.step_count) == ou.STEPS and int(opt.skipped) == 0
    assert all(r <= 2.0 for r in worst_ratio.values())


# ------------------------------------------------------------------------------------------------- norm and clip
@pytest.mark.parametrize("case", ["below", "above", "none"])
def test_grad_norm_and_clip_coef(case):
    params, grads = ou.trajectory_inputs(1, seed=11)
    G = grads[0]
    exact = math.sqrt(math.fsum(float(x) * float(x) for g in G for x in g.reshape(-1).astype(np.float64)))
    max_norm = {"below": 2.0 * exact, "above": 0.37 * exact, "none": None}[case]
    tp, opt = _device_adam(params, max_norm=max_norm)
    _set_grads(tp, opt, G)
    opt.step()
    n_chunks = sum((g.size + CHUNK - 1) // CHUNK for g in G)
    path = 16 + 8 + (n_chunks + 255) // 256 + 8
    rel = abs(float(opt.grad_norm) - exact) / exact
    print(f"max_norm {case}: grad_norm {float(opt.grad_norm):.17g} vs exact {exact:.17g}, rel err {rel:.2e}"
          f" (bound {(path + 2) * 2.0 ** -53:.2e}, path {path} additions over {n_chunks} chunks)")
    assert opt.grad_norm.dtype == torch.float64 and rel <= (path + 2) * 2.0 ** -53
    model = ou.AdamModel(params, LR, BETAS, EPS, max_norm)
    model.step(G)
    want = {"below": 1.0, "none": 1.0}.get(case, float(model.clip_coef))
    assert float(model.clip_coef) == want and (case != "above" or 0.36 < want < 0.38)
    assert float(opt.clip_coef) == want


# ------------------------------------------------------------------------------------------------- edges
EDGE_SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
VIEW_AT, NONE_AT = len(EDGE_SIZES), 2              # the misaligned view's index; the parameter that loses its gradient


def test_edges_of_the_chunk_table():
    """Segment lengths on both sides of the 16-byte vector, of a wave (64 lanes, and 64 quads = 256), of a chunk; one
    parameter that is a view starting one float into its storage (misaligned: the scalar body); 70 segments in all; and in
    the third step one parameter without a gradient."""
    rng = np.random.default_rng(21)
    sizes = EDGE_SIZES + [300] + [7 + (i % 5) for i in range(70 - len(EDGE_SIZES) - 1)]
    assert len(sizes) == 70
    params = [rng.normal(0, 0.05, n).astype(np.float32) for n in sizes]
    grads = [[rng.normal(0, 10.0 ** rng.uniform(-3, -1), n).astype(np.float32) for n in sizes] for _ in range(3)]
    grads[2][NONE_AT] = None

    from pixel_nerf_multiscale_amd.optim import DeviceAdam
    tp = [torch.nn.Parameter(torch.from_numpy(p.copy()).cuda()) for p in params]
    storage = torch.full((sizes[VIEW_AT] + 2,), 777.0, device="cuda")
    storage[1:-1] = torch.from_numpy(params[VIEW_AT]).cuda()
    tp[VIEW_AT] = torch.nn.Parameter(storage[1:-1])
    assert tp[VIEW_AT].data_ptr() % 16 == 4 and tp[VIEW_AT].is_contiguous()
    opt = DeviceAdam(tp, lr=LR, betas=BETAS, eps=EPS, max_norm=MAX_NORM)

    model = ou.AdamModel(params, LR, BETAS, EPS, MAX_NORM)
    ttp, topt, tstep = ou.torch_adam_cpu(params)
    for k, G in enumerate(grads):
        before = _state(tp, opt)
        _set_grads(tp, opt, G)
        opt.step()
        model.step(G)
        tstep(G)
        assert float(opt.clip_coef) == float(model.clip_coef), k
    after = _state(tp, opt)
    for a, b in zip(before, after):                 # the parameter without a gradient kept its bits in the last step ..
        assert _same_bits([a[NONE_AT]], [b[NONE_AT]])
        assert not _same_bits([a[NONE_AT + 1]], [b[NONE_AT + 1]])          # .. while its neighbours moved
    assert float(storage[0]) == 777.0 and float(storage[-1]) == 777.0       # nothing written around the view
    assert int(opt.step_count) == 3
    _compare("edges, 70 segments, 3 steps", after, ou.torch_state(ttp, topt), (model.p, model.m, model.v))


# ------------------------------------------------------------------------------------------------- non-finite gradients
SCALER = dict(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)


@pytest.mark.parametrize("where", ["inf_last_of_last", "nan_first_of_first"])
@pytest.mark.parametrize("with_scaler", [True, False])
def test_non_finite_gradient_skips_the_step(where, with_scaler):
    """The non-finite values are inputs of a guarded kernel: the step is skipped on the device, with or without a scaler."""
    params, grads = ou.trajectory_inputs(5, seed=5)
    tp, opt = _device_adam(params, scaler=SCALER if with_scaler else None)
    s0 = 1024.0 if with_scaler else 1.0
    scaled = lambda G, s: [(g * np.float32(s)).astype(np.float32) for g in G]
    _set_grads(tp, opt, scaled(grads[0], s0))
    opt.step()                                      # one clean step: m, v non-zero
    assert int(opt.step_count) == 1 and int(opt.growth_tracker) == (1 if with_scaler else 0) and float(opt.scale_value) == s0
    before = _state(tp, opt)
    bad = scaled(grads[1], s0)
    if where == "inf_last_of_last":
        bad[-1].reshape(-1)[-1] = np.inf
    else:
        bad[0].reshape(-1)[0] = np.nan
    _set_grads(tp, opt, bad)
    opt.step()
    after = _state(tp, opt)
    assert all(_same_bits(a, b) for a, b in zip(before, after))             # every bit of p, m, v
    assert int(opt.found_inf) == 1 and int(opt.step_count) == 1 and int(opt.skipped) == 1
    assert not math.isfinite(float(opt.grad_norm))
    if with_scaler:
        assert float(opt.scale_value) == 512.0 and int(opt.growth_tracker) == 0
        model = ou.AdamModel(params, LR, BETAS, EPS, MAX_NORM, scaler=SCALER)
        model.step(scaled(grads[0], 1024.0))
        model.step(bad)
        for k in range(3):                          # the scale doubles after three clean steps and not before
            assert float(opt.scale_value) == 512.0 and int(opt.growth_tracker) == k
            _set_grads(tp, opt, scaled(grads[2 + k], 512.0))
            opt.step()
            model.step(scaled(grads[2 + k], 512.0))
            assert int(opt.found_inf) == 0
        assert float(opt.scale_value) == 1024.0 == float(model.scale) and int(opt.growth_tracker) == 0
        assert int(opt.step_count) == 4 == model.t and int(opt.skipped) == 1
        # the scale is a power of two, so the scaled run is the plain run: same bound against the same model
        ttp, topt, tstep = ou.torch_adam_cpu(params)
        for k in (0, 2, 3, 4):
            tstep(grads[k])
        _compare(f"scaler, skip at step 2 ({where})", _state(tp, opt), ou.torch_state(ttp, topt), (model.p, model.m, model.v))
    else:
        assert float(opt.scale_value) == 1.0 and int(opt.growth_tracker) == 0
        _set_grads(tp, opt, grads[2])
        opt.step()
        assert int(opt.found_inf) == 0 and int(opt.step_count) == 2 and int(opt.skipped) == 1


def test_scale_multiplies_the_loss_on_the_device():
    params, _ = ou.trajectory_inputs(1, seed=5)
    tp, opt = _device_adam(params[:3], scaler=SCALER)
    loss = (tp[1] * tp[1]).sum()
    scaled = opt.scale(loss)
    assert scaled.is_cuda and float(scaled.detach()) == 1024.0 * float(loss.detach())
    opt.zero_grad()
    scaled.backward()
    assert tp[1].grad.data_ptr() == opt._slice_ptr[1]                       # accumulated where step() reads
    assert torch.equal(tp[1].grad, 2048.0 * tp[1].detach())
    tp2, opt2 = _device_adam(params[:3])
    assert opt2.scale(loss) is loss


# ------------------------------------------------------------------------------------------------- determinism
def test_two_runs_give_the_same_bits():
    params, grads = ou.trajectory_inputs(3, seed=8)
    runs = []
    for _ in range(2):
        tp, opt = _device_adam(params, scaler=SCALER)
        for G in grads:
            _set_grads(tp, opt, [(g * np.float32(1024.0)).astype(np.float32) for g in G])
            opt.step()
        runs.append((_state(tp, opt), opt._state_buf.cpu().numpy().copy()))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert _same_bits(a, b)
    assert np.array_equal(runs[0][1], runs[1][1])                           # the whole state record


# ------------------------------------------------------------------------------------------------- .grad handling
def test_a_replaced_gradient_is_adopted_again():
    params, grads = ou.trajectory_inputs(1, seed=9)
    params, G = params[:6], grads[0][:6]
    tp, opt = _device_adam(params)
    tp2, opt2 = _device_adam(params)
    _set_grads(tp, opt, G)
    for t in tp2:
        t.grad = None                               # what zero_grad(set_to_none=True) of another optimizer leaves ..
    for t, g in zip(tp2, G):
        t.grad = torch.from_numpy(g).view_as(t).cuda()                      # .. and backward then allocates
    opt.step()
    opt2.step()
    for i, t in enumerate(tp2):
        assert t.grad.data_ptr() == opt2._slice_ptr[i]
    for a, b in zip(_state(tp, opt), _state(tp2, opt2)):
        assert _same_bits(a, b)
    opt2.zero_grad(set_to_none=True)                # ignored: one memset, the views stay
    assert all(t.grad is not None and t.grad.data_ptr() == opt2._slice_ptr[i] and not bool(t.grad.any()) for i, t in enumerate(tp2))


# ------------------------------------------------------------------------------------------------- checkpoints, schedulers
def test_state_dict_round_trip_through_torch_adam():
    """DeviceAdam -> torch.optim.Adam -> DeviceAdam, one step taken in each, against an uninterrupted run: after each step
    the mixed run is within 2x of the error torch's own uninterrupted run has at that step."""
    params, grads, err, snaps = ou.torch_reference()
    tp, opt = _device_adam(params)
    _set_grads(tp, opt, grads[0])
    opt.step()
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(len(params))) and float(sd["state"][0]["step"]) == 1.0
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["scaler"] is None

    cp = [torch.nn.Parameter(t.detach().cpu().clone()) for t in tp]
    adam = torch.optim.Adam(cp, lr=123.0, foreach=False)
    adam.load_state_dict(sd)
    assert adam.param_groups[0]["lr"] == LR and adam.param_groups[0]["betas"] == BETAS
    for t, g in zip(cp, grads[1]):
        t.grad = torch.from_numpy(g.copy()).view_as(t)
    torch.nn.utils.clip_grad_norm_(cp, MAX_NORM)
    adam.step()
    mixed = ou.torch_state(cp, adam)
    for q, a in zip("pmv", mixed):
        print(f"after Adam's step: max |{q} - model| {ou.worst(a, snaps[1][q]):.3e}  torch alone {err[1][q]:.3e}")
        assert ou.worst(a, snaps[1][q]) <= 2.0 * err[1][q], q

    tp2, opt2 = _device_adam([t.detach().numpy() for t in cp], lr=55.0)
    opt2.load_state_dict(adam.state_dict())
    assert int(opt2.step_count) == 2 and opt2.param_groups[0]["lr"] == LR
    _set_grads(tp2, opt2, grads[2])
    opt2.step()
    assert int(opt2.step_count) == 3
    for q, a in zip("pmv", _state(tp2, opt2)):
        print(f"after DeviceAdam's step: max |{q} - model| {ou.worst(a, snaps[2][q]):.3e}  torch alone {err[2][q]:.3e}")
        assert ou.worst(a, snaps[2][q]) <= 2.0 * err[2][q], q

    # the scaler entry survives a round trip of its own
    tp3, opt3 = _device_adam(params[:4], scaler=SCALER)
    _set_grads(tp3, opt3, [(g * np.float32(1024.0)).astype(np.float32) for g in grads[0][:4]])
    opt3.step()
    sd3 = opt3.state_dict()
    assert sd3["scaler"]["scale"] == 1024.0 and sd3["scaler"]["growth_tracker"] == 1
    tp4, opt4 = _device_adam([t.detach().cpu().numpy() for t in tp3], scaler=SCALER)
    opt4.load_state_dict(sd3)
    assert float(opt4.scale_value) == 1024.0 and int(opt4.growth_tracker) == 1 and int(opt4.step_count) == 1
    for a, b in zip(_state(tp3, opt3), _state(tp4, opt4)):
        assert _same_bits(a, b)


def test_step_lr_changes_the_applied_lr():
    params, grads = ou.trajectory_inputs(2, seed=13)
    tp, opt = _device_adam(params[:5])
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)
    model = ou.AdamModel(params[:5], LR, BETAS, EPS, MAX_NORM)
    ttp, topt, tstep = ou.torch_adam_cpu(params[:5])
    tsched = torch.optim.lr_scheduler.StepLR(topt, step_size=1, gamma=0.1)
    want = [np.float32(LR / (1 - 0.9)), np.float32(LR * 0.1 / (1 - 0.9 ** 2))]
    for k in range(2):
        _set_grads(tp, opt, grads[k][:5])
        opt.step()
        sched.step()
        model.step(grads[k][:5], lr=LR * 0.1 ** k)
        tstep(grads[k][:5])
        tsched.step()
        assert float(opt.step_size) == float(want[k]), k
    assert abs(opt.param_groups[0]["lr"] - LR * 0.01) <= 1e-12
    _compare("StepLR, 2 steps", _state(tp, opt), ou.torch_state(ttp, topt), (model.p, model.m, model.v))


# ------------------------------------------------------------------------------------------------- train.train_step
def test_train_step_end_to_end():
    """One step on the smallest golden case of test_gpu_train_front (tiny_ns2_codeview, 2 objects x 32 rays) by two routes
    from the same seeds: train.train_step with DeviceAdam, and calc_losses, backward, clip_grad_norm_,
    torch.optim.Adam.step.  The gradients of both are the same bits; each route's parameters are compared with the fp64
    model's step from those gradients, and the device route may be at most 2x as far from it as torch's."""
    from pixel_nerf_multiscale_amd import train
    from pixel_nerf_multiscale_amd.model.loss import RenderLoss
    from pixel_nerf_multiscale_amd.optim import DeviceAdam
    from test_gpu_train_front import LAM_C, LAM_F, RAY_BATCH, Z_FAR, Z_NEAR, _front_end_setup
    kw = dict(ray_batch_size=RAY_BATCH, nviews=[2], z_near=Z_NEAR, z_far=Z_FAR, loss=RenderLoss(LAM_C, LAM_F))
    max_norm = 0.01

    def named(net):
        return [(f"{w}.{k}", p) for w, mlp in (("coarse", net.mlp_coarse), ("fine", net.mlp_fine)) for k, p in mlp.named_parameters()]

    # the torch route
    net, rend, data, kept = _front_end_setup()
    names, tparams = zip(*named(net))
    start = [p.detach().cpu().numpy().copy() for p in tparams]
    adam = torch.optim.Adam(tparams, lr=LR, betas=BETAS, eps=EPS)
    torch.manual_seed(7); np.random.seed(7)
    adam.zero_grad(set_to_none=True)
    loss, _ = train.calc_losses(net, rend.bind_parallel(net, None), data, **kw)
    loss.backward()
    tgrads = [p.grad.detach().cpu().numpy().copy() for p in tparams]
    tnorm = float(torch.nn.utils.clip_grad_norm_(tparams, max_norm))
    adam.step()
    torch_p = [p.detach().cpu().numpy() for p in tparams]

    # the device route
    net2, rend2, data2, kept2 = _front_end_setup()
    dparams = [p for _, p in named(net2)]
    assert all(np.array_equal(a, p.detach().cpu().numpy()) for a, p in zip(start, dparams))
    opt = DeviceAdam(dparams, lr=LR, betas=BETAS, eps=EPS, max_norm=max_norm)
    render_par = rend2.bind_parallel(net2, None)
    hooked = []
    torch.manual_seed(3); np.random.seed(3)
    with torch.no_grad():
        train.calc_losses(net2, render_par, data2, **kw)            # warm-up of the front end: allocations, code objects
    works = sync_debug_mode_works()
    print(f'torch.cuda.set_sync_debug_mode("error") works under this build: {works}')
    torch.manual_seed(7); np.random.seed(7)
    if works:
        torch.cuda.set_sync_debug_mode("error")
    try:
        d = train.train_step(net2, render_par, data2, opt, grad_hook=lambda: hooked.append(1), **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert hooked == [1]
    assert sorted(d) == ["grad_norm", "rc", "rf", "t"] and all(v.is_cuda and v.dim() == 0 for v in d.values())
    assert d["grad_norm"].dtype == torch.float64 and int(opt.step_count) == 1 and int(opt.found_inf) == 0
    assert float(d["t"]) == float(loss.detach())

    dgrads = [p.grad.detach().cpu().numpy() for p in dparams]        # never written back: still what backward left
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(tgrads, dgrads))
    model = ou.AdamModel(start, LR, BETAS, EPS, max_norm)
    model.step(dgrads)
    rel = abs(float(d["grad_norm"]) - model.grad_norm) / model.grad_norm
    print(f"grad_norm {float(d['grad_norm']):.9g} (clip_grad_norm_ {tnorm:.9g}), rel err vs fp64 {rel:.2e}; clip_coef {float(opt.clip_coef):.6g}")
    assert rel <= 64 * 2.0 ** -53 and abs(tnorm - model.grad_norm) <= 1e-5 * model.grad_norm
    assert model.clip_coef < 1.0 and float(opt.clip_coef) == float(model.clip_coef)
    dev_p = [p.detach().cpu().numpy() for p in dparams]
    ek, et = ou.worst(dev_p, model.p), ou.worst(torch_p, model.p)
    moved = ou.worst(start, model.p)
    print(f"train_step: max |p - model|  device route {ek:.3e}  torch route {et:.3e}  ratio {ek / et:.2f}  (the step moved p by {moved:.3e})")
    assert moved > 100 * et and ek <= 2.0 * et
