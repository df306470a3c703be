"""CPU-side checks of the linear-kernel suite (tests/test_gpu_train_gemm.py): its case table reaches every launch site the
dispatchers record, every recorded site is a real launch, the table spans the edges it claims, the debug entry's argument
struct matches the header, and the fp64 bound has the power to reject the defects tile GEMMs actually have."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

import train_gemm_util as U


def test_case_table_reaches_every_launch_site():
    reached = {c["kernel"] for c in U.CASES}
    assert reached == set(U.KERNEL_IDS), set(U.KERNEL_IDS) ^ reached
    assert sorted(U.KERNEL_IDS.values()) == list(range(1, len(U.KERNEL_IDS) + 1))
    assert U.header_enum("PNR_DBG_K_")["COUNT"] == len(U.KERNEL_IDS) + 1


def test_every_kernel_id_names_a_real_launch_site():
    """Each PNR_DBG_K_* is recorded exactly once in csrc/train_f32.hip, right in front of the launch of the kernel it names."""
    src = open(U.SOURCE).read()
    expect = {
        "SGEMM_DMA_WT": "k_sgemm_dma<", "MGEMM_BF16X3": "k_mgemm_bf16x3<", "MGEMM_BF16": "k_mgemm_bf16<", "SGEMM_DMA": "k_sgemm_dma<",
        "MGEMM_F32": "k_mgemm_f32<", "LINEAR_HEAD_512": "k_linear_head<", "LINEAR_HEAD_256": "k_linear_head<",
        "GEMM_F32": "k_gemm_f32<", "HGEMM_DMA_M16": "k_hgemm_dma<", "HGEMM_DMA": "k_hgemm_dma<",
        "MGEMM_BF16_A16_M16": "k_mgemm_bf16<true", "MGEMM_BF16_A16": "k_mgemm_bf16<true", "MGEMM_BF16_M16": "k_mgemm_bf16<true",
        "MGEMM_BF16_G16": "k_mgemm_bf16<true", "HEAD_DX": "k_head_dx", "COL_SUMS16": "k_col_sums16", "COL_SUMS": "k_col_sums",
        "GRAD_W_SKINNY48": "k_grad_w_skinny<48>", "GRAD_W_SKINNY96": "k_grad_w_skinny<", "MGEMM_BF16X3_DW": "k_mgemm_bf16x3<",
        "HGEMM_DMA_KT": "k_hgemm_dma_kt<", "MGEMM_BF16_DW_A16B16": "k_mgemm_bf16<false",
        "MGEMM_BF16_DW_B16": "k_mgemm_bf16<false", "MGEMM_BF16_DW": "k_mgemm_bf16<",
        "SGEMM_DMA_KT": "k_sgemm_dma_kt<", "MGEMM_F32_DW": "k_mgemm_f32<false", "GRAD_W_HEAD": "k_grad_w_head<",
        "GRAD_W_F32": "k_grad_w_f32<",
    }
    assert set(expect) == set(U.KERNEL_IDS)
    for name in U.KERNEL_IDS:
        sites = [m.end() for m in re.finditer(r"\bPNR_DBG_K_%s\b" % name, src)]
        assert len(sites) == 1, (name, len(sites))
        # (a record that chooses between two sites by the launch's own condition precedes both launches)
        nxt = [m.group(0) for m in re.finditer(r"hipLaunchKernelGGL\(\(?[^,]*", src[sites[0]:])][:2]
        assert any(expect[name] in n for n in nxt), (name, nxt)


def test_case_table_spans_the_edges():
    Ms = {c["M"] for c in U.CASES}
    assert {1, 31, 63, 64, 127, 129, 255, 1000, 40000} <= Ms and max(Ms) > 64 * 1024
    assert {4, 32, 96, 128, 160, 512} <= {c["N"] for c in U.CASES}
    assert {4, 16, 32, 39, 48, 64, 96, 128, 160, 256, 512} <= {c["K"] for c in U.CASES}
    assert any(c["ws"] for c in U.CASES) and any(c["offx"] or c["offy"] for c in U.CASES)
    assert any((c["ldy"] or 0) % 4 for c in U.CASES) and any(c["ldx"] and c["ldx"] > c["K"] for c in U.CASES)
    assert {c["epi"] for c in U.CASES} >= {"LDS", "LDS_C16", "REG_VEC", "REG_ELEM"}
    names = [c["name"] for c in U.CASES + U.SIBLING_CASES]
    assert len(names) == len(set(names))


def test_debug_args_struct_matches_header():
    from pixel_nerf_multiscale_amd import _native as N
    fields = [f for f, _ in N.pnr_debug_linear_args._fields_]
    body = ", ".join(f"(long)offsetof(pnr_debug_linear_args, {f})" for f in fields)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "pnr.h"\nint main(){long o[] = {%s};\n'
           'printf("%%zu", sizeof(pnr_debug_linear_args)); for (unsigned i = 0; i < sizeof(o) / sizeof(o[0]); ++i) printf(" %%ld", o[i]);'
           'return 0;}\n' % body)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(U.ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(N.pnr_debug_linear_args)
    assert got[1:] == [getattr(N.pnr_debug_linear_args, f).offset for f in fields]


def _fp32_product(a, b):
    """An honest fp32 product (CPU BLAS, fp32 accumulation) standing in for a kernel."""
    return a.float() @ b.float().T


@pytest.mark.parametrize("M,N,K", [(129, 96, 256), (63, 160, 512)])
def test_bound_rejects_subtly_wrong_products(M, N, K):
    """The bound has power: an honest fp32 product passes it, a product with ONE term dropped, with one 64-deep k-step
    dropped, or a weight gradient with one padding row counted twice fails it by a wide margin."""
    g = torch.Generator().manual_seed(M * N + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    y = _fp32_product(x, w) + b
    v, bound, _ = U.reference(x, w, bias=b)
    ok = U.worst_ratio(y, v, bound)
    assert ok <= 0.5, ok
    # one product term dropped: the (i, j, k) with the median-sized |x w| of row i
    i, j = M // 2, N // 3
    t = (x[i].double() * w[j].double())
    k = int(t.abs().argsort()[K // 2])
    y1 = y.clone()
    y1[i, j] = float(y[i, j].double() - t[k])
    assert U.worst_ratio(y1, v, bound) > 10
    # one 64-deep k-step skipped (the last one)
    y2 = _fp32_product(x[:, :K - 64], w[:, :K - 64]) + b
    assert U.worst_ratio(y2, v, bound) > 100
    # dW = g^T x with the last row counted twice (a clamped re-read of a padding row that was not zeroed)
    G = torch.randn(M, N, generator=g)
    dW = _fp32_product(G.T, x.T)
    vw, bw, _ = U.reference(G.T, x.T)
    assert U.worst_ratio(dW, vw, bw) <= 0.5
    dW3 = dW + torch.outer(G[-1], x[-1])
    assert U.worst_ratio(dW3, vw, bw) > 100


def test_bf16_bound_uses_the_rounded_operands():
    """Against the rounded operands the bf16 product is held to the fp32 bound; against the fp32 operands it is not (the
    reference must round the operands the way the kernel does)."""
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(64, 256, generator=g), torch.randn(128, 256, generator=g)
    xr, wr = U.bf16_round(x), U.bf16_round(w)
    y = _fp32_product(xr, wr)
    v, bound, _ = U.reference(xr, wr)
    assert U.worst_ratio(y, v, bound) <= 0.5
    v2, bound2, _ = U.reference(x, w)
    assert U.worst_ratio(y, v2, bound2) > 10
