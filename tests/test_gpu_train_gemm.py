"""The training path's linear-layer kernels one product at a time, through the production dispatchers (pnr_debug_linear), against
an fp64 product of the operands they multiply (tests/train_gemm_util.py: table, reference, bound).

Every case asserts the launch site it must reach first (a case cannot pass on a fallback), then
  - |y - y64| <= 2 gamma_{K+2} (|act x| |w|^T + |b| + |r|) elementwise (+ 2^-14 |x| |w|^T for bf16x3),
  - masked entries are exactly 0 before r is added, the bf16 copy is the round-to-nearest-even of the kernel's own y,
  - nothing outside the matrices is written, and nothing outside them is read (the gaps of every strided operand hold NaN).
Row counts off the tile multiples (1, 31, 63, 127, 129, 255, 1000), widths at the dispatch predicates' edges, leading
dimensions wider than the row, odd leading dimensions and base offsets of 1-2 elements, split counts up to the cap and
scratch-starved slicing of the weight gradients.  Observed worst error / bound per case on an MI355X: 1e-6 to 0.23 for
every output held in fp32 (k_head_dx / k_gemm_f32 at K = 4 the highest, the long dW sums the lowest); 0.96-0.98 for the cases
whose result leaves only as its bf16 copy (noY: the copy's own rounding, up to 2^-8 relative, is part of that bound)."""
import ctypes as C

import pytest
import torch

import train_gemm_util as U

pytestmark = pytest.mark.gpu
NAN16 = 0x7FC0


def _lib():
    from pixel_nerf_multiscale_amd import _native as N
    return N


def _mat(rows, cols, ld, off, dtype, dev, values):
    """A (rows, cols) matrix at element offset `off` of a flat buffer with leading dimension ld; every other element of the
    buffer is NaN (fp32) / 0x7FC0 (bf16 bits).  Returns (buffer, matrix view)."""
    n = off + rows * ld + 8
    if dtype == torch.int16:
        buf = torch.full((n,), NAN16, dtype=torch.int16, device=dev)
    else:
        buf = torch.full((n,), float("nan"), dtype=dtype, device=dev)
    view = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    if values is not None:
        view.copy_(values)
    return buf, view


def _bits16(t):
    """bf16 images of fp32 values as int16 bits (RNE)."""
    return t.to(torch.bfloat16).view(torch.int16)


def _val16(bits):
    return bits.view(torch.bfloat16).float()


def _mask_values(g, shape, dev):
    """A relu mask with 0, -0, negatives and tiny positives (normal and subnormal)."""
    m = torch.randn(shape, generator=g, device=dev)
    u = torch.rand(shape, generator=g, device=dev)
    m = torch.where(u < 0.08, torch.zeros_like(m), m)
    m = torch.where((u >= 0.08) & (u < 0.14), torch.full_like(m, -0.0), m)
    m = torch.where((u >= 0.14) & (u < 0.18), torch.full_like(m, 1e-30), m)
    m = torch.where((u >= 0.18) & (u < 0.20), torch.full_like(m, 1e-40), m)
    return m


def _mask16_bits(g, shape, dev):
    b = _bits16(_mask_values(g, shape, dev))
    u = torch.rand(shape, generator=g, device=dev)
    b = torch.where(u < 0.03, torch.full_like(b, 0x0001), b)              # smallest positive bf16 (subnormal): kept
    b = torch.where((u >= 0.03) & (u < 0.06), torch.full_like(b, -0x7FFF), b)   # 0x8001: negative, dropped
    return b


def run_case(c, seed=1234):
    """Runs one table row; returns a dict of what it checked (ratio, the outputs)."""
    N_ = _lib()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(seed)
    op, mode, M, N, K = c["op"], c["mode"], c["M"], c["N"], c["K"]
    o = c["opts"]
    kern = c["kernel"]
    bf16 = kern in U.BF16_KERNELS
    x3 = kern in U.X3_KERNELS
    a = N_.pnr_debug_linear_args()
    a.op, a.mode, a.relu, a.m, a.n, a.k = U.OP[op], mode, c["relu"], M, N, K
    keep = []                                             # buffers alive until the call has finished
    res = {}

    if op in ("FWD", "DX", "HEAD_DX"):
        Kx = K
        ldx = c["ldx"] or Kx
        X = torch.randn(M, Kx, generator=g, device=dev)
        if op == "FWD":
            W = torch.randn(N, K, generator=g, device=dev) / K ** 0.5
            ldw = c["ldw"] or K
            wbuf, wv = _mat(N, K, ldw, 0, torch.float32, dev, W)
        else:                                             # W stored (K, N): y = x . W
            W = torch.randn(K, N, generator=g, device=dev) / K ** 0.5
            ldw = c["ldw"] or N
            wbuf, wv = _mat(K, N, ldw, 0, torch.float32, dev, W)
        a.w, a.ldw = wbuf.data_ptr(), ldw
        keep.append(wbuf)
        if "X16" in o:
            xbuf, xv = _mat(M, Kx, ldx, c["offx"], torch.int16, dev, _bits16(X))
            a.x16 = xbuf.data_ptr() + 2 * c["offx"]
            xs = _val16(xv)
        else:
            xs = None
        xbuf32, _ = _mat(M, Kx, ldx, c["offx"], torch.float32, dev, X)
        a.x = xbuf32.data_ptr() + 4 * c["offx"]
        a.ldx = ldx
        keep += [xbuf32] + ([xbuf] if "X16" in o else [])
        if "W16" in o:
            wt = W if op == "FWD" else W.t().contiguous()        # (N, K), leading dimension K
            if mode == U.T16:
                w16 = _bits16(wt).contiguous()
                a.w16 = w16.data_ptr()
            else:
                w16 = wt.contiguous()
                a.w16 = w16.data_ptr()
            keep.append(w16)
        # operands as the kernel multiplies them
        xa = X if xs is None else xs
        wn = W if op == "FWD" else W.t()                          # (N, K)
        if bf16:
            xa = U.bf16_round(xa)
            wn = U.bf16_round(wn)
        b = torch.randn(N, generator=g, device=dev) if "b" in o else None
        if b is not None:
            a.b = b.data_ptr()
            keep.append(b)
        ldr = c["ldr"] or N
        R = torch.randn(M, N, generator=g, device=dev) if "R" in o else None
        if R is not None:
            rbuf, _ = _mat(M, N, ldr, 0, torch.float32, dev, R)
            a.r, a.ldr = rbuf.data_ptr(), ldr
            keep.append(rbuf)
        ldm = c["ldm"] or N
        mk = mk16 = None
        if "Mk" in o:
            mk = _mask_values(g, (M, N), dev)
            mbuf, _ = _mat(M, N, ldm, 0, torch.float32, dev, mk)
            a.mk = mbuf.data_ptr()
            keep.append(mbuf)
        if "Mk16" in o:
            mk16 = _mask16_bits(g, (M, N), dev)
            mbuf16, _ = _mat(M, N, ldm, 0, torch.int16, dev, mk16)
            a.mk16 = mbuf16.data_ptr()
            keep.append(mbuf16)
        a.ldm = ldm
        ldy = c["ldy"] or N
        ybuf, yv = _mat(M, N, ldy, c["offy"], torch.float32, dev, None)
        if "noY" not in o:
            a.y = ybuf.data_ptr() + 4 * c["offy"]
        a.ldy = ldy
        if "Y16" in o:
            y16buf, y16v = _mat(M, N, ldy, c["offy"], torch.int16, dev, None)
            a.y16 = y16buf.data_ptr() + 2 * c["offy"]
        rc = N_.lib.pnr_debug_linear(C.byref(a), N_.current_stream(dev))
        torch.cuda.synchronize()
        assert rc == 0, (c["name"], rc)
        assert U.KERNEL_NAMES.get(a.kernel) == kern, (c["name"], U.KERNEL_NAMES.get(a.kernel), kern)
        if c["epi"] is not None:
            assert a.epilogue == U.EPI[c["epi"]], (c["name"], a.epilogue, c["epi"])
        relu = bool(c["relu"]) and op == "FWD"
        v, bound, kp = U.reference(xa, wn, relu=relu, bias=b, mk=mk, mk16=mk16, r=R, x3=x3)
        if "noY" not in o:
            y = yv
            res["ratio"] = U.worst_ratio(y, v, bound)
            if kp is not None:                         # masked entries: exactly 0 before r is added
                base = R if R is not None else torch.zeros_like(y)
                assert torch.equal(y[~kp], base[~kp]), c["name"]
            gap = ybuf.clone()
            gap[c["offy"]:c["offy"] + M * ldy].view(M, ldy)[:, :N] = float("nan")
            assert torch.isnan(gap).all(), (c["name"], "y written outside the matrix")
            res["y"] = y.clone()
        if "Y16" in o:
            y16 = y16v
            if "noY" not in o:                         # the bf16 copy is the RNE of the kernel's own y
                assert torch.equal(y16, _bits16(yv)), c["name"]
            else:
                r16 = U.worst_ratio(_val16(y16), v, bound + 2.0 ** -8 * (v.abs() + bound))
                res["ratio"] = r16
                if kp is not None:
                    assert (_val16(y16)[~kp] == 0).all(), c["name"]
            gap = y16buf.clone()
            gap[c["offy"]:c["offy"] + M * ldy].view(M, ldy)[:, :N] = NAN16
            assert (gap == NAN16).all(), (c["name"], "y16 written outside the matrix")
            res["y16"] = y16.clone()
    else:                                                 # DW: y (N, K) += g^T act(x), db += sum g
        ldx = c["ldx"] or K
        ldg = c["ldg"] or N
        X = torch.randn(M, K, generator=g, device=dev)
        G = torch.randn(M, N, generator=g, device=dev) * 0.5
        gbuf, _ = _mat(M, N, ldg, 0, torch.float32, dev, G)
        a.g, a.ldg = gbuf.data_ptr(), ldg
        keep.append(gbuf)
        if "G16" in o:
            g16buf, g16v = _mat(M, N, ldg, 0, torch.int16, dev, _bits16(G))
            a.g16 = g16buf.data_ptr()
            keep.append(g16buf)
        xbuf, _ = _mat(M, K, ldx, c["offx"], torch.float32, dev, X)
        a.x, a.ldx = xbuf.data_ptr() + 4 * c["offx"], ldx
        keep.append(xbuf)
        if "X16" in o:
            x16buf, x16v = _mat(M, K, ldx, c["offx"], torch.int16, dev, _bits16(X))
            a.x16 = x16buf.data_ptr() + 2 * c["offx"]
            keep.append(x16buf)
        ga, xa = G, X
        if bf16:
            ga, xa = U.bf16_round(G), U.bf16_round(X)
        if kern == "COL_SUMS16":                      # the column sums of the gradient stream's bf16 copy
            ga = U.bf16_round(G)
        if c["relu"]:
            xa = xa.clamp_min(0.0)
        ldy = c["ldy"] or K
        dW0 = torch.randn(N, K, generator=g, device=dev)
        ybuf, yv = _mat(N, K, ldy, 0, torch.float32, dev, dW0)
        if "nodW" not in o:
            a.y, a.ldy = ybuf.data_ptr(), ldy
        db0 = torch.randn(N, generator=g, device=dev)
        dbt = db0.clone()
        if "db" in o:
            a.db = dbt.data_ptr()
        ws_floats = c["ws"] or 64 * (N * K + N)
        ws = torch.full((ws_floats,), float("nan"), device=dev)
        a.ws, a.ws_floats = ws.data_ptr(), ws_floats
        rc = N_.lib.pnr_debug_linear(C.byref(a), N_.current_stream(dev))
        torch.cuda.synchronize()
        assert rc == 0, (c["name"], rc)
        assert U.KERNEL_NAMES.get(a.kernel) == kern, (c["name"], U.KERNEL_NAMES.get(a.kernel), kern)
        if c["splits"] is not None:
            lo, hi = c["splits"]
            assert lo <= a.splits <= hi, (c["name"], a.splits, a.rows_per_split)
        assert a.splits * (N * K + N) <= ws_floats and (a.splits - 1) * a.rows_per_split < M <= a.splits * a.rows_per_split
        ratio = 0.0
        if "nodW" not in o:
            v, bound, _ = U.reference(ga.t(), xa.t(), acc0=dW0, x3=x3)
            ratio = U.worst_ratio(yv, v, bound)
            gap = ybuf.clone()
            gap[:N * ldy].view(N, ldy)[:, :K] = float("nan")
            assert torch.isnan(gap).all(), (c["name"], "dW written outside the matrix")
            res["y"] = yv.clone()
        else:
            assert torch.isnan(ybuf[:N * ldy].view(N, ldy)[:, K:]).all()
        if "db" in o:
            v, bound, _ = U.reference(ga.t(), torch.ones(1, M, device=dev), acc0=db0[:, None], x3=x3)
            ratio = max(ratio, U.worst_ratio(dbt[:, None], v, bound))
            res["db"] = dbt.clone()
        else:
            assert torch.equal(dbt, db0)
        res["ratio"] = ratio
        res["splits"], res["rows"] = a.splits, a.rows_per_split
    res["kernel"], res["epilogue"] = a.kernel, a.epilogue
    print(f"{c['name']}: {kern} epilogue={a.epilogue} splits={a.splits} worst err/bound = {res['ratio']:.3g}")
    return res


@pytest.mark.parametrize("c", U.CASES, ids=[c["name"] for c in U.CASES])
def test_linear_kernel_against_fp64(c):
    res = run_case(c)
    assert res["ratio"] <= 1.0, (c["name"], res["ratio"])


@pytest.mark.parametrize("i", range(len(U.SIBLINGS)), ids=[s[0] for s in U.SIBLINGS])
def test_sibling_kernels_bit_identical(i):
    """The pairs the code comments call bit-identical, on the same operand values, the dispatcher steered to each side by
    W16 present / absent, a leading dimension or a base offset only."""
    _, ca, cb = U.SIBLINGS[i]
    ra, rb = run_case(ca, seed=99 + i), run_case(cb, seed=99 + i)
    assert ra["ratio"] <= 1.0 and rb["ratio"] <= 1.0
    keys = [k for k in ("y", "y16", "db") if k in ra]
    assert keys and keys == [k for k in ("y", "y16", "db") if k in rb]
    for k in keys:
        assert torch.equal(ra[k], rb[k]), (U.SIBLINGS[i][0], k, float((ra[k].float() - rb[k].float()).abs().max()))


def test_sgemm_dma_is_not_held_to_mgemm_f32_bits():
    """k_sgemm_dma groups its sums differently from k_mgemm_f32 (documented as not bit-identical): both held to the bound."""
    a = U.case("pair_sdma", "FWD", U.F32, 1000, 512, 512, "SGEMM_DMA", "b", "R", relu=1)
    b = U.case("pair_mf32", "FWD", U.F32, 1000, 512, 512, "MGEMM_F32", "b", "R", relu=1, offx=1)
    assert run_case(a, seed=5)["ratio"] <= 1.0 and run_case(b, seed=5)["ratio"] <= 1.0


def _copy(op, x, m, k=0, ldx=0, y16t=False):
    N_ = _lib()
    dev = x.device
    a = N_.pnr_debug_linear_args()
    a.op, a.m, a.k, a.ldx = U.OP[op], m, k, ldx
    a.x = x.data_ptr()
    n_out = m if op == "TO_BF16" else m * k
    y = torch.full((n_out + 8,), 0x1234, dtype=torch.int16, device=dev)
    a.y16 = y.data_ptr()
    yt = None
    if y16t:
        yt = torch.full((n_out + 8,), 0x1234, dtype=torch.int16, device=dev)
        a.y16t = yt.data_ptr()
    assert N_.lib.pnr_debug_linear(C.byref(a), N_.current_stream(dev)) == 0
    torch.cuda.synchronize()
    assert (y[n_out:] == 0x1234).all() and (yt is None or (yt[n_out:] == 0x1234).all())
    return y[:n_out], (yt[:n_out] if yt is not None else None)


def _special_values(dev, n=4096):
    g = torch.Generator(device=dev).manual_seed(7)
    base = torch.randn(n, generator=g, device=dev) * torch.exp2(torch.randint(-140, 120, (n,), generator=g, device=dev).float())
    ties = (torch.arange(1, 257, device=dev, dtype=torch.int32) << 16) | 0x8000        # exactly half an ulp of bf16: ties
    ties2 = ((torch.arange(1, 257, device=dev, dtype=torch.int32) + 0x3F00) << 16) | 0x8000
    specials = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.4028235e38, -3.4028235e38, 1e-40, -1e-40,
                             1.401298e-45, 9.1835e-41, 1.1754942e-38, 1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8, 1.0 + 2 ** -8 + 2 ** -20],
                            device=dev)
    return torch.cat([base, ties.view(torch.float32), ties2.view(torch.float32), -ties2.view(torch.float32), specials])


def _assert_rne(got_bits, x):
    want = x.to(torch.bfloat16).view(torch.int16)
    nan = torch.isnan(x)
    assert torch.isnan(got_bits[nan].view(torch.bfloat16)).all()
    bad = (got_bits != want) & ~nan
    assert not bad.any(), (x[bad][:8].tolist(), got_bits[bad][:8].tolist(), want[bad][:8].tolist())


def test_bf16_copy_kernels_are_round_to_nearest_even():
    """k_to_bf16, k_cols_to_bf16 and k_w_to_bf16 (plain and transposed) bit-equal to torch's RNE on ties, +-0, subnormals,
    +-Inf, values that round to Inf; NaN stays NaN."""
    dev = torch.device("cuda")
    x = _special_values(dev)
    y, _ = _copy("TO_BF16", x, x.numel())
    _assert_rne(y, x)
    rows, L, ld = x.numel() // 64, 62, 66                 # the first L columns of a wider row
    xm = torch.full((rows, ld), float("nan"), device=dev)
    xm[:, :L] = x[:rows * L].view(rows, L)
    y, _ = _copy("COLS_TO_BF16", xm, rows, L, ld)
    _assert_rne(y.view(rows, L), xm[:, :L])
    R_, C_ = 37, x.numel() // 37
    w = x[:R_ * C_].reshape(R_, C_).contiguous()
    y, yt = _copy("W_TO_BF16", w, R_, C_, y16t=True)
    _assert_rne(y.view(R_, C_), w)
    _assert_rne(yt.view(C_, R_), w.t())


def test_nan_in_the_relu_mask_fp32_drops_bf16_keeps_positive():
    """The two mask forms differ on NaN (mgemm_epilogue documents it): the fp32 mask keeps m > 0, so NaN drops the entry; the
    bf16 mask keeps 'sign clear and nonzero', so a positive-sign NaN keeps it and a negative-sign NaN drops it."""
    N_ = _lib()
    dev = torch.device("cuda")
    M, N, K = 64, 128, 64
    g = torch.Generator(device=dev).manual_seed(3)
    X = torch.randn(M, K, generator=g, device=dev)
    W = torch.randn(N, K, generator=g, device=dev)
    out = {}
    for form in ("fp32", "bf16"):
        a = N_.pnr_debug_linear_args()
        a.op, a.mode, a.m, a.n, a.k = U.OP["FWD"], U.T16, M, N, K
        x16, w16 = _bits16(X), _bits16(W)
        a.x16, a.w16, a.w, a.x, a.ldx, a.ldw = x16.data_ptr(), w16.data_ptr(), W.data_ptr(), X.data_ptr(), K, K
        if form == "fp32":
            mk = torch.ones(M, N, device=dev)
            mk[:, 0] = float("nan")
            mk[:, 1] = -float("nan")
            a.mk = mk.data_ptr()
        else:
            mk = torch.full((M, N), 0x3F80, dtype=torch.int16, device=dev)
            mk[:, 0] = 0x7FC0
            mk[:, 1] = -64                                 # 0xFFC0: negative-sign NaN
            a.mk16 = mk.data_ptr()
        a.ldm = N
        y = torch.full((M, N), float("nan"), device=dev)
        a.y, a.ldy = y.data_ptr(), N
        assert N_.lib.pnr_debug_linear(C.byref(a), N_.current_stream(dev)) == 0
        torch.cuda.synchronize()
        out[form] = y
    ref = U.bf16_round(X).double() @ U.bf16_round(W).double().T
    assert (out["fp32"][:, :2] == 0).all()
    assert (out["bf16"][:, 1] == 0).all()
    assert (out["bf16"][:, 0].double() - ref[:, 0]).abs().max() <= 1e-3 * ref.abs().max()
    assert torch.equal(out["fp32"][:, 2:], out["bf16"][:, 2:])


def test_hgemm_dma_beyond_4_gib_of_activations():
    """k_hgemm_dma with M * ldx * 2 > 2^32 bytes: the first, the last and 2000 random rows against fp64."""
    N_ = _lib()
    dev = torch.device("cuda")
    M, N, K = (1 << 22) + 4096 + 37, 128, 512
    assert M * K * 2 > 2 ** 32
    g = torch.Generator(device=dev).manual_seed(11)
    x16 = torch.randn(M, K, generator=g, device=dev, dtype=torch.bfloat16)
    W = torch.randn(N, K, generator=g, device=dev) / K ** 0.5
    w16 = _bits16(W)
    b = torch.randn(N, generator=g, device=dev)
    y = torch.empty(M, N, device=dev)
    try:
        a = N_.pnr_debug_linear_args()
        a.op, a.mode, a.relu, a.m, a.n, a.k = U.OP["FWD"], U.T16, 1, M, N, K
        a.x16, a.ldx, a.w16, a.w, a.ldw, a.b, a.y, a.ldy = x16.data_ptr(), K, w16.data_ptr(), W.data_ptr(), K, b.data_ptr(), \
            y.data_ptr(), N
        assert N_.lib.pnr_debug_linear(C.byref(a), N_.current_stream(dev)) == 0
        torch.cuda.synchronize()
        assert U.KERNEL_NAMES[a.kernel] == "HGEMM_DMA"
        rows = torch.cat([torch.tensor([0, 1, M - 2, M - 1], device=dev),
                          torch.randint(0, M, (2000,), generator=g, device=dev),
                          torch.arange(M - 200, M, device=dev)])
        v, bound, _ = U.reference(x16[rows].float(), _val16(w16), relu=True, bias=b)
        r = U.worst_ratio(y[rows], v, bound)
        print(f"hgemm_dma > 4 GiB: worst err/bound = {r:.3g}")
        assert r <= 1.0
    finally:
        del x16, y
        torch.cuda.empty_cache()
