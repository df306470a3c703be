"""fp64 model of the training back end's arithmetic, written from include/pnr.h (the text, not csrc/optim.hip):

    unscaled = fp32(grad * inv_scale)                       inv_scale = fp32(1 / scale), 1 without a scaler
    total    = sqrt(sum unscaled^2)                         clip_coef = fp32(min(1, max_norm / (total + 1e-6))), 1 for max_norm <= 0
    g        = unscaled * clip_coef
    m' = beta1 m + (1 - beta1) g      v' = beta2 v + (1 - beta2) g^2
    p' = p - lr / (1 - beta1^t) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)         t counted AFTER its increment
    non-finite unscaled gradient: nothing moves, skipped += 1, with or without a scaler
    scaler: non-finite -> scale *= backoff, tracker = 0; finite -> tracker + 1, at growth_interval: scale *= growth, tracker = 0

Everything after the two fp32 roundings that DEFINE the inputs (the unscaled gradient, which is what clip_grad_norm_ sees, and
clip_coef, which the kernel publishes as fp32) is fp64: the model is the exact value an fp32 implementation is measured
against.  `mutation` breaks one rule at a time, for the tests that show the checks can tell."""
import functools

import numpy as np

LR, BETAS, EPS, MAX_NORM, STEPS = 1e-4, (0.9, 0.999), 1e-8, 0.05, 40
# max_norm = 0.05 sits inside the range of norms the gradient scales 1e-4 .. 10 give (0.017 .. 1700 over 29 k elements): some
# steps are not clipped, most are, and just above max_norm the 1e-6 of the clip is 2e-5 of the coefficient — visible in fp32.
SIZES = [1, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 512 * 42]       # the 13 tensors of the trajectory tests
SHAPES = [(n,) for n in SIZES[:-1]] + [(512, 42)]
MUTATIONS = ("swapped_betas", "no_bias_correction", "eps_under_root", "no_clip_eps", "step_counts_skips")


class AdamModel:
    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=None, scaler=None, mutation=None):
        assert mutation is None or mutation in MUTATIONS
        self.p = [np.asarray(p, dtype=np.float64).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.lr, self.betas, self.eps, self.max_norm = lr, betas, eps, max_norm
        self.mutation = mutation
        self.t = 0
        self.skipped = 0
        self.scaler = None if scaler is None else dict(scaler)
        self.scale = np.float32(scaler["init_scale"]) if scaler else np.float32(1.0)
        self.tracker = 0
        self.grad_norm = 0.0
        self.clip_coef = np.float32(1.0)
        self.found_inf = 0

    def _scaler_update(self, found):
        if self.scaler is None:
            return
        if found:
            self.scale = np.float32(self.scale * np.float32(self.scaler["backoff_factor"]))
            self.tracker = 0
        else:
            self.tracker += 1
            if self.tracker >= self.scaler["growth_interval"]:
                self.scale = np.float32(self.scale * np.float32(self.scaler["growth_factor"]))
                self.tracker = 0

    def step(self, grads, lr=None):
        """grads: fp32 arrays (None = no gradient for that tensor this step), as backward left them (still scaled)."""
        lr = self.lr if lr is None else lr
        inv = np.float32(1.0 / np.float64(self.scale)) if self.scaler is not None else np.float32(1.0)
        with np.errstate(all="ignore"):
            un = [None if g is None else (np.asarray(g, dtype=np.float32) * inv).astype(np.float32) for g in grads]
            total = float(np.sqrt(sum(float((u.astype(np.float64) ** 2).sum()) for u in un if u is not None)))
        found = int(not np.isfinite(total) or any(u is not None and not np.isfinite(u).all() for u in un))
        self.grad_norm, self.found_inf = total, found
        if found:
            self.clip_coef = np.float32(0.0)
            self.skipped += 1
            if self.mutation == "step_counts_skips":
                self.t += 1
            self._scaler_update(True)
            return
        coef = 1.0
        if self.max_norm is not None and self.max_norm > 0:
            coef = min(1.0, self.max_norm / (total + (0.0 if self.mutation == "no_clip_eps" else 1e-6)))
        self.clip_coef = np.float32(coef)
        self.t += 1
        b1, b2 = self.betas if self.mutation != "swapped_betas" else self.betas[::-1]
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        if self.mutation == "no_bias_correction":
            bc1 = bc2 = 1.0
        for i, u in enumerate(un):
            if u is None:
                continue
            g = u.astype(np.float64).reshape(self.p[i].shape) * np.float64(self.clip_coef)
            self.m[i] = b1 * self.m[i] + (1.0 - b1) * g
            self.v[i] = b2 * self.v[i] + (1.0 - b2) * g * g
            if self.mutation == "eps_under_root":
                den = np.sqrt(self.v[i] / bc2 + self.eps)
            else:
                den = np.sqrt(self.v[i]) / np.sqrt(bc2) + self.eps
            self.p[i] = self.p[i] - (lr / bc1) * self.m[i] / den
        self._scaler_update(False)


def trajectory_inputs(steps=40, seed=0):
    """The shared case: 13 tensors (SHAPES), `steps` gradients whose scale runs over 1e-4 .. 10 (both sides of max_norm = 1)."""
    rng = np.random.default_rng(seed)
    params = [rng.normal(0, 0.05, s).astype(np.float32) for s in SHAPES]
    grads = []
    for _ in range(steps):
        amp = 10.0 ** rng.uniform(-4, 1)
        grads.append([rng.normal(0, amp, s).astype(np.float32) for s in SHAPES])
    return params, grads


def worst(arrs, ref):
    """max |a - ref| over a list of arrays, in fp64."""
    return max(float(np.abs(np.asarray(a, dtype=np.float64).reshape(r.shape) - r).max()) for a, r in zip(arrs, ref))


def torch_adam_cpu(params, m=None, v=None, step=0, lr=LR, max_norm=MAX_NORM):
    """torch.optim.Adam(foreach=False) on CPU fp32 copies of `params`, optionally resumed from moments and a step count.
    -> (parameter list, optimizer, step function taking fp32 gradient arrays (None allowed) and returning clip_grad_norm_'s norm)."""
    import torch
    tp = [torch.nn.Parameter(torch.from_numpy(np.asarray(p, dtype=np.float32).copy())) for p in params]
    opt = torch.optim.Adam(tp, lr=lr, betas=BETAS, eps=EPS, foreach=False)
    if m is not None:
        for t, a, b in zip(tp, m, v):
            opt.state[t] = {"step": torch.tensor(float(step)), "exp_avg": torch.from_numpy(np.asarray(a, dtype=np.float32).copy()),
                            "exp_avg_sq": torch.from_numpy(np.asarray(b, dtype=np.float32).copy())}

    def do_step(G):
        for t, g in zip(tp, G):
            t.grad = None if g is None else torch.from_numpy(np.asarray(g, dtype=np.float32).copy()).view_as(t)
        norm = 0.0
        if max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(tp, max_norm))
        opt.step()
        return norm

    return tp, opt, do_step


def torch_state(tp, opt):
    """-> p, m, v lists (numpy fp32) of a torch Adam; zeros where it holds no state yet."""
    p = [t.detach().numpy().copy() for t in tp]
    m = [opt.state[t]["exp_avg"].numpy().copy() if t in opt.state and opt.state[t] else np.zeros_like(x) for t, x in zip(tp, p)]
    v = [opt.state[t]["exp_avg_sq"].numpy().copy() if t in opt.state and opt.state[t] else np.zeros_like(x) for t, x in zip(tp, p)]
    return p, m, v


@functools.lru_cache(maxsize=None)
def torch_reference():
    """torch's Adam + clip_grad_norm_ over the shared trajectory on the CPU in fp32, next to the fp64 model: per step torch's
    error against the model (p, m, v), the model's state, and torch's norm.  Computed once per process and left unchanged."""
    params, grads = trajectory_inputs(STEPS)
    tp, opt, do_step = torch_adam_cpu(params)
    model = AdamModel(params, LR, BETAS, EPS, MAX_NORM)
    err, snaps, gmax = [], [], 0.0
    for G in grads:
        norm = do_step(G)
        model.step(G)
        gmax = max(gmax, max(float(np.abs(g).max()) for g in G) * float(model.clip_coef))
        tpn, tm, tv = torch_state(tp, opt)
        err.append({"p": worst(tpn, model.p), "m": worst(tm, model.m), "v": worst(tv, model.v)})
        snaps.append({"p": [a.copy() for a in model.p], "m": [a.copy() for a in model.m], "v": [a.copy() for a in model.v],
                      "gmax": gmax, "pmax": max(float(np.abs(a).max()) for a in model.p), "torch_norm": norm,
                      "norm": model.grad_norm, "clip_coef": model.clip_coef})
    return params, grads, err, snaps
