#!/usr/bin/env python3
"""Timing of the training step's back end — what follows loss.backward(): unscale, clip_grad_norm_, the optimizer step, the
scaler's update, zero_grad — on the real parameter set (both ResnetFC and the ResNet-34 trunk up to layer 3, ~14 M parameters
in ~150 tensors), at tools/bench_train.py's bf16 1- and 2-view configuration.  Timed in the same run, in alternating rounds,
medians reported:
  tail_torch        GradScaler.unscale_, clip_grad_norm_, scaler.step(torch.optim.Adam), scaler.update, zero_grad(set_to_none)
  tail_torch_fused  the same with Adam(fused=True), when this torch has it
  tail_device       optim.DeviceAdam: step() (three launches) and zero_grad() (one memset)
  grads_assign      what the two torch tails pay in this tool only: pointing .grad at stand-in gradients again after
                    zero_grad(set_to_none=True) dropped them (in training, backward allocates them)
  step_*            the whole step (render forward with the tape, loss, backward, tail) with each tail
One JSON line per view count.
The torch tails unscale and clip their gradients in place, so the stand-in gradients, handed back every iteration, shrink by
the scale each time and are zero or denormal after a few iterations; tail_device copies those values into its own buffer.
None of the tails branches on a finite value (the passes are bandwidth- or launch-bound), so the timing does not depend on it.
    python tools/bench_optim.py [--sb 4] [--rays 128] [--views 1 2] [--steps 20] [--tail-steps 400] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_util as gu  # noqa: E402
import hip_util as hu  # noqa: E402

GRAD_CLIP = 1.0
SCALER = dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)


def trainable(net):
    """Both MLPs and the trunk as far as the latent maps use it (layer4 and fc feed nothing)."""
    out = []
    for k, p in net.named_parameters():
        if p.requires_grad and not (k.startswith("encoder.") and (".layer4." in k or ".fc." in k)):
            out.append(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sb", type=int, default=4)
    ap.add_argument("--rays", type=int, default=128)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tail-steps", type=int, default=400,
                    help="iterations of a timed window of the tail_* and grads_assign variants: a tail is 0.1-2 ms, so a window of "
                         "--steps of them would measure the clock and the scheduler")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optim.py measures on the GPU; there is none here")
    from pixel_nerf_multiscale_amd.optim import DeviceAdam

    for ns in a.views:
        spec = gu._case(seed=5, d_hidden=512, lat=[(256, 8, 8)], image=(128, 128), focal=131.25, NS=ns, SB=a.sb,
                        N=a.rays, Kc=64, Kf=32, Kfd=16)
        rays_np, poses_np = gu.make_inputs(spec)
        net = hu.build_net(spec, poses_np).train()
        net.train_precision = "bf16"
        maps = [torch.from_numpy(x).cuda().requires_grad_(True) for x in gu.make_latents(spec)]
        net.encoder.set_latents(maps)
        rend = hu.build_renderer(spec)
        rays = torch.from_numpy(rays_np).cuda()
        tgt = torch.rand(a.sb, a.rays, 3, device="cuda")

        params = trainable(net)
        mlp_ids = {id(p) for m in (net.mlp_coarse, net.mlp_fine) if m is not None for p in m.parameters()}
        trunk = [p for p in params if id(p) not in mlp_ids]
        n_param = sum(p.numel() for p in params)
        gen = torch.Generator(device="cuda").manual_seed(1)
        stand_in = [torch.randn(p.shape, device="cuda", generator=gen) * (1e-3 * SCALER["init_scale"]) for p in params]

        trunk_g = [g for p, g in zip(params, stand_in) if id(p) not in mlp_ids]

        adam = torch.optim.Adam(params, lr=1e-4)
        tails = {"torch": (adam, torch.amp.GradScaler("cuda", **SCALER))}
        try:
            tails["torch_fused"] = (torch.optim.Adam(params, lr=1e-4, fused=True), torch.amp.GradScaler("cuda", **SCALER))
        except (TypeError, RuntimeError) as e:
            print(f"# Adam(fused=True) is not available here: {e}", file=sys.stderr)
        for _, sc in tails.values():
            sc.scale(torch.zeros((), device="cuda"))      # GradScaler creates its device scale at the first scale() call
        dev = DeviceAdam(params, lr=1e-4, max_norm=GRAD_CLIP, scaler=SCALER)

        def assign(ps=params, gs=stand_in):
            for p, g in zip(ps, gs):
                p.grad = g

        def torch_tail(opt, scaler):
            scaler.unscale_(opt)
            torch.nn.utils.clip_grad_norm_(params, GRAD_CLIP)
            scaler.step(opt)
            scaler.update()
            opt.zero_grad(set_to_none=True)

        def device_tail():
            dev.step()
            dev.zero_grad()

        def loss_of(out):
            return ((out.coarse.rgb - tgt) ** 2).mean() + ((out.fine.rgb - tgt) ** 2).mean()

        def step_torch(opt, scaler):
            scaler.scale(loss_of(rend(net, rays, want_weights=True))).backward()
            assign(trunk, trunk_g)           # the trunk's gradients: the fixed latent maps of this workload produce none
            torch_tail(opt, scaler)

        def step_device():
            dev.scale(loss_of(rend(net, rays, want_weights=True))).backward()
            dev.step()
            dev.zero_grad()

        variants = {"grads_assign": (assign, None)}
        for k, (opt, sc) in tails.items():
            variants["tail_" + k] = (lambda opt=opt, sc=sc: (assign(), torch_tail(opt, sc)), None)
        variants["tail_device"] = (device_tail, dev.attach_grads)
        for k, (opt, sc) in tails.items():
            variants["step_" + k] = (lambda opt=opt, sc=sc: step_torch(opt, sc), lambda: [setattr(p, "grad", None) for p in params])
        variants["step_device"] = (step_device, lambda: (dev.attach_grads(), dev.zero_grad()))

        def run(name, n):
            fn, prepare = variants[name]
            if prepare is not None:
                prepare()
            if name == "tail_device":       # stand-in gradients in the optimizer's own buffer (see the note on their values above)
                for p, g in zip(params, stand_in):
                    p.grad.copy_(g)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        n_of = {k: (a.steps if k.startswith("step_") else a.tail_steps) for k in variants}
        for k in variants:
            run(k, a.warmup)
        ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k in variants:
                ms[k].append(run(k, n_of[k]))
        med = {k: statistics.median(v) for k, v in ms.items()}
        res = {"what": "train_back_end", "sb": a.sb, "rays_per_obj": a.rays, "views": ns, "precision": "bf16", "tensors": len(params),
               "parameters": n_param, "steps": a.steps, "tail_steps": a.tail_steps,
               "rounds": a.rounds}
        res.update({"ms_" + k: round(v, 4) for k, v in med.items()})
        res.update({"spread_ms_" + k: round(max(v) - min(v), 4) for k, v in ms.items()})
        res["device_tail_bytes"] = (4 + 28 + 4) * n_param            # norm pass 4 B, update 28 B, memset 4 B per parameter
        res["device_tail_tb_per_s"] = round(res["device_tail_bytes"] / (med["tail_device"] * 1e-3) / 1e12, 3)
        best = min(v for k, v in med.items() if k.startswith("tail_torch"))
        res["device_tail_faster_than_torchs_best"] = med["tail_device"] < best
        res["skipped_steps_device"] = int(dev.skipped)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
