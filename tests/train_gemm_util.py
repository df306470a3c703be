"""Case table, fp64 reference and error bound of the training path's linear-layer products (csrc/train_f32.hip: gemm, gemm16,
grad_w, head_dx), shared by tests/test_gpu_train_gemm.py (the kernels through pnr_debug_linear) and
tests/test_train_gemm_cpu.py (table coverage and the power of the bound, no GPU).

Every product has a plain meaning — y = mask(act(x) w^T + b) + r, or dW += g^T act(x), db += sum g — so an fp64 product of the
operands the kernel multiplies is an exact reference: the fp32 values (fp32 and bf16x3 products), or their round-to-nearest-even
bf16 images (the bf16 modes; relu commutes with the rounding).  What remains is fp32 accumulation, bounded elementwise by
    |y - y64| <= 2 gamma_{K+2} (|act x| |w|^T + |b| + |r|),   gamma_n = n 2^-24
(K: the reduction length; for dW the rows M, with |dW0| / |db0| for the accumulated values), and for bf16x3 by
2^-14 |x| |w|^T more (the dropped lo*lo term and the rounding of the lo parts)."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pnr.h")
SOURCE = os.path.join(ROOT, "pixel_nerf_multiscale_amd", "csrc", "train_f32.hip")


def header_enum(prefix):
    txt = open(HEADER).read()
    return {m.group(1)[len(prefix):]: int(m.group(2)) for m in re.finditer(r"\b(%s[A-Z0-9_]+)\s*=\s*(\d+)" % prefix, txt)}


KERNEL_IDS = {k: v for k, v in header_enum("PNR_DBG_K_").items() if k not in ("NONE", "COUNT")}
KERNEL_NAMES = {v: k for k, v in KERNEL_IDS.items()}
EPI = header_enum("PNR_DBG_EPI_")
OP = header_enum("PNR_DBG_OP_")
F32, BF16, X3, T16 = 0, 1, 3, 16

# the kernels whose products run on rounded bf16 operands, and the bf16x3 ones
BF16_KERNELS = {"HGEMM_DMA", "HGEMM_DMA_M16", "MGEMM_BF16", "MGEMM_BF16_A16", "MGEMM_BF16_A16_M16", "MGEMM_BF16_M16",
                "MGEMM_BF16_G16", "HGEMM_DMA_KT", "MGEMM_BF16_DW_A16B16", "MGEMM_BF16_DW_B16", "MGEMM_BF16_DW"}
X3_KERNELS = {"MGEMM_BF16X3", "MGEMM_BF16X3_DW"}


def case(name, op, mode, M, N, K, kernel, *opts, relu=0, ldx=None, ldw=None, ldy=None, ldg=None, ldr=None, ldm=None, offx=0,
         offy=0, ws=None, epi=None, splits=None):
    """One row of the table.  op: FWD / DX / HEAD_DX / DW; mode: F32, BF16, X3 (gemm / grad_w's `half`) or T16 (gemm16);
    kernel: the PNR_DBG_K_* the dispatcher must take.  opts: b, R, Mk (fp32 mask), Mk16 (bf16 mask), X16, W16 (gemm16's W16 /
    the dX products' W^T copy), Y16, noY (only the bf16 copy of y leaves), db, nodW, G16 (dW: the bf16 copy of dY).
    ld* default to the row length; offx / offy: base offsets in elements of x (x16) / y (y16); ws: scratch floats of a weight
    gradient (default: the library's DET_MAX_SPLITS slices); epi: the PNR_DBG_EPI_* a forward / dX tile kernel must take;
    splits: (min, max) of the row slices a weight gradient must use."""
    assert kernel in KERNEL_IDS, kernel
    assert set(opts) <= {"b", "R", "Mk", "Mk16", "X16", "W16", "Y16", "noY", "db", "nodW", "G16"}, opts
    return dict(name=name, op=op, mode=mode, M=M, N=N, K=K, kernel=kernel, opts=frozenset(opts), relu=relu, ldx=ldx, ldw=ldw,
                ldy=ldy, ldg=ldg, ldr=ldr, ldm=ldm, offx=offx, offy=offy, ws=ws, epi=epi, splits=splits)


E = EPI
CASES = [
    # ---------------- forward, fp32 products (gemm<RELU_X, false>)
    case("fwd_f32_dma_m1", "FWD", F32, 1, 512, 512, "SGEMM_DMA", "b", epi="LDS"),
    case("fwd_f32_dma_m31_relu", "FWD", F32, 31, 128, 64, "SGEMM_DMA", "b", "R", relu=1, epi="LDS"),
    case("fwd_f32_dma_m63_mask", "FWD", F32, 63, 160, 128, "SGEMM_DMA", "b", "Mk", "R", epi="LDS"),
    case("fwd_f32_dma_m64", "FWD", F32, 64, 96, 256, "SGEMM_DMA", "b", epi="LDS"),
    case("fwd_f32_dma_m127_n32", "FWD", F32, 127, 32, 512, "SGEMM_DMA", "Mk", relu=1, epi="LDS"),
    case("fwd_f32_dma_m129", "FWD", F32, 129, 512, 512, "SGEMM_DMA", "b", "Mk", "R", relu=1, epi="LDS"),
    case("fwd_f32_dma_m1000_ldy_odd", "FWD", F32, 1000, 160, 96, "SGEMM_DMA", "b", "R", ldy=161, ldr=163, epi="REG_ELEM"),
    case("fwd_f32_dma_n150_regvec", "FWD", F32, 255, 150, 64, "SGEMM_DMA", "b", "R", "Mk", ldy=152, ldr=152, ldm=152,
         epi="REG_VEC"),
    case("fwd_f32_dma_wide_ldx", "FWD", F32, 1000, 512, 256, "SGEMM_DMA", "b", relu=1, ldx=256 + 44, epi="LDS"),
    case("fwd_f32_mfma_k39", "FWD", F32, 255, 512, 39, "MGEMM_F32", "b", relu=1, ldx=42, epi="REG_VEC"),
    case("fwd_f32_mfma_k48", "FWD", F32, 129, 96, 48, "MGEMM_F32", "b", "Mk", "R", epi="REG_VEC"),
    case("fwd_f32_mfma_offx1", "FWD", F32, 1000, 128, 512, "MGEMM_F32", "b", "R", relu=1, offx=1, epi="REG_VEC"),
    case("fwd_f32_mfma_k16_ldy_odd", "FWD", F32, 63, 32, 16, "MGEMM_F32", "b", "Mk", ldy=33, epi="REG_ELEM"),
    case("fwd_head_512", "FWD", F32, 1000, 4, 512, "LINEAR_HEAD_512", "b", relu=1),
    case("fwd_head_256", "FWD", F32, 129, 4, 256, "LINEAR_HEAD_256", relu=1, ldx=260),
    case("fwd_fma_n4_k39", "FWD", F32, 255, 4, 39, "GEMM_F32", "b", relu=1, ldx=42),
    case("fwd_fma_head_with_r", "FWD", F32, 127, 4, 512, "GEMM_F32", "b", "R", relu=1),
    # ---------------- forward, bf16 / bf16x3 products on the fp32 tape (gemm's half = 1 / 3)
    case("fwd_bf16_m1", "FWD", BF16, 1, 512, 512, "MGEMM_BF16", "b", relu=1, epi="REG_VEC"),
    case("fwd_bf16_m129_k96", "FWD", BF16, 129, 160, 96, "MGEMM_BF16", "b", "Mk", "R", epi="REG_VEC"),
    case("fwd_bf16_m1000_k32", "FWD", BF16, 1000, 32, 32, "MGEMM_BF16", "b", relu=1, ldy=35, epi="REG_ELEM"),
    case("fwd_x3_m255", "FWD", X3, 255, 512, 160, "MGEMM_BF16X3", "b", "Mk", "R", relu=1, epi="REG_VEC"),
    case("fwd_x3_m63_n96", "FWD", X3, 63, 96, 512, "MGEMM_BF16X3", "b", epi="REG_VEC"),
    # ---------------- forward, 16-bit tape (gemm16<RELU_X, false>)
    case("fwd_t16_dma_m1", "FWD", T16, 1, 128, 64, "HGEMM_DMA", "X16", "W16", "b", "Y16", relu=1, epi="LDS"),
    case("fwd_t16_dma_m31", "FWD", T16, 31, 512, 512, "HGEMM_DMA", "X16", "W16", "b", "R", "Y16", epi="LDS"),
    case("fwd_t16_dma_m129_n160", "FWD", T16, 129, 160, 128, "HGEMM_DMA", "X16", "W16", "b", "R", relu=1, epi="LDS"),
    case("fwd_t16_dma_m1000_c16only", "FWD", T16, 1000, 512, 256, "HGEMM_DMA_M16", "X16", "W16", "b", "Mk16", "Y16", "noY",
         relu=1, epi="LDS_C16"),
    case("fwd_t16_dma_m255_mask16", "FWD", T16, 255, 96, 512, "HGEMM_DMA_M16", "X16", "W16", "b", "Mk16", "R", "Y16", epi="LDS"),
    case("fwd_t16_dma_ldy_odd", "FWD", T16, 127, 160, 64, "HGEMM_DMA_M16", "X16", "W16", "b", "Mk16", "R", "Y16", ldy=163,
         ldr=161, epi="REG_ELEM"),
    case("fwd_t16_dma_offy1", "FWD", T16, 255, 128, 256, "HGEMM_DMA", "X16", "W16", "b", "R", "Y16", offy=1, epi="REG_ELEM"),
    case("fwd_t16_dma_wide_ldx", "FWD", T16, 1000, 512, 256, "HGEMM_DMA", "X16", "W16", "b", "Y16", ldx=256 + 48, epi="LDS"),
    case("fwd_t16_a16_k96", "FWD", T16, 255, 512, 96, "MGEMM_BF16_A16", "X16", "W16", "b", "R", "Y16", relu=1, epi="REG_VEC"),
    case("fwd_t16_a16_k160_m16", "FWD", T16, 129, 128, 160, "MGEMM_BF16_A16_M16", "X16", "W16", "b", "Mk16", "Y16", "noY",
         epi="REG_VEC"),
    case("fwd_t16_m16_f32x", "FWD", T16, 63, 160, 128, "MGEMM_BF16_M16", "b", "Mk16", "R", relu=1, ldx=132, epi="REG_VEC"),
    case("fwd_t16_g16_mk32", "FWD", T16, 1000, 96, 64, "MGEMM_BF16_G16", "b", "Mk", "R", "Y16", epi="REG_VEC"),
    # ---------------- dX (gemm<false, true>, gemm16<false, true>), the output head's dX
    case("dx_f32_wt_m1", "DX", F32, 1, 512, 512, "SGEMM_DMA_WT", "W16", "Mk", epi="LDS"),
    case("dx_f32_wt_m1000", "DX", F32, 1000, 512, 128, "SGEMM_DMA_WT", "W16", "Mk", epi="LDS"),
    case("dx_f32_wt_ldy_odd", "DX", F32, 129, 96, 64, "SGEMM_DMA_WT", "W16", "Mk", ldy=97, epi="REG_ELEM"),
    case("dx_f32_mfma_m255", "DX", F32, 255, 512, 512, "MGEMM_F32", "Mk", epi="REG_VEC"),
    case("dx_f32_mfma_k39", "DX", F32, 63, 160, 39, "MGEMM_F32", "Mk", ldx=40, epi="REG_VEC"),
    case("dx_f32_fma_k4", "DX", F32, 1000, 512, 4, "GEMM_F32", "Mk"),
    case("dx_bf16_m127", "DX", BF16, 127, 512, 128, "MGEMM_BF16", "Mk", epi="REG_VEC"),
    case("dx_t16_dma_m129", "DX", T16, 129, 512, 512, "HGEMM_DMA_M16", "X16", "W16", "Mk16", "Y16", epi="LDS"),
    case("dx_t16_dma_m1000", "DX", T16, 1000, 128, 256, "HGEMM_DMA", "X16", "W16", "Y16", "noY", epi="LDS_C16"),
    # an fp32 mask keeps the bf16 operands off the DMA kernel (it takes the bf16 mask only)
    case("dx_t16_a16_mk32", "DX", T16, 1000, 128, 256, "MGEMM_BF16_A16", "X16", "W16", "Mk", "Y16", "noY", epi="REG_VEC"),
    case("dx_t16_a16_m129", "DX", T16, 129, 512, 512, "MGEMM_BF16_A16_M16", "X16", "Mk16", "Y16", epi="REG_VEC"),
    case("head_dx_n512", "HEAD_DX", F32, 1000, 512, 4, "HEAD_DX", "Mk", "Y16"),
    case("head_dx_n128_m1", "HEAD_DX", F32, 1, 128, 4, "HEAD_DX", "Mk"),
    case("head_dx_n512_nomask", "HEAD_DX", F32, 129, 512, 4, "HEAD_DX"),
    # ---------------- dW / db (grad_w<RELU_X>)
    case("dw_colsums", "DW", F32, 1000, 512, 512, "COL_SUMS", "nodW", "db"),
    case("dw_colsums16", "DW", BF16, 4097, 160, 512, "COL_SUMS16", "nodW", "db", "G16"),
    case("dw_skinny48_m1000", "DW", F32, 1000, 512, 39, "GRAD_W_SKINNY48", "db", ldx=42),
    case("dw_skinny48_bf16mode", "DW", BF16, 127, 64, 4, "GRAD_W_SKINNY48", "db"),
    case("dw_skinny96_m40000", "DW", X3, 40000, 512, 78, "GRAD_W_SKINNY96", "db", ldx=80),
    case("dw_skinny96_nodb", "DW", F32, 31, 128, 96, "GRAD_W_SKINNY96"),
    case("dw_x3_m1000", "DW", X3, 1000, 512, 512, "MGEMM_BF16X3_DW", "db", relu=1),
    case("dw_x3_m63_k96", "DW", X3, 63, 96, 96, "MGEMM_BF16X3_DW", relu=1),
    case("dw_hkt_m64", "DW", BF16, 64, 128, 128, "HGEMM_DMA_KT", "X16", "G16", "db", relu=1, splits=(1, 1)),
    case("dw_hkt_m40000", "DW", BF16, 40000, 512, 512, "HGEMM_DMA_KT", "X16", "G16", "db", relu=1, splits=(32, 32)),
    case("dw_hkt_m4096_nodb", "DW", BF16, 4096, 256, 512, "HGEMM_DMA_KT", "X16", "G16", relu=1),
    case("dw_hkt_starved", "DW", BF16, 40000, 128, 256, "HGEMM_DMA_KT", "X16", "G16", "db", relu=1,
         ws=3 * (128 * 256 + 128), splits=(3, 3)),
    case("dw_a16b16_m1000", "DW", BF16, 1000, 512, 512, "MGEMM_BF16_DW_A16B16", "X16", "G16", "db", relu=1),
    case("dw_a16b16_m96", "DW", BF16, 96, 128, 128, "MGEMM_BF16_DW_A16B16", "X16", "G16", "db", relu=1),
    case("dw_a16b16_m129_n160", "DW", BF16, 129, 160, 96, "MGEMM_BF16_DW_A16B16", "X16", "G16", "db"),
    case("dw_a16b16_m31", "DW", BF16, 31, 128, 128, "MGEMM_BF16_DW_A16B16", "X16", "G16", "db", relu=1),
    case("dw_a16b16_ldx_wide", "DW", BF16, 4096, 256, 512, "MGEMM_BF16_DW_A16B16", "X16", "G16", "db", relu=1, ldx=516),
    case("dw_b16_m255", "DW", BF16, 255, 512, 512, "MGEMM_BF16_DW_B16", "X16", "db", relu=1),
    case("dw_bf16_m1000", "DW", BF16, 1000, 160, 128, "MGEMM_BF16_DW", "db", relu=1),
    case("dw_bf16_m70000", "DW", BF16, 70001, 128, 128, "MGEMM_BF16_DW", "db", relu=1, splits=(35, 35)),
    case("dw_sdkt_m32", "DW", F32, 32, 128, 128, "SGEMM_DMA_KT", "db", relu=1),
    case("dw_sdkt_m40000", "DW", F32, 40000, 512, 512, "SGEMM_DMA_KT", "db", relu=1, splits=(32, 32)),
    case("dw_sdkt_starved", "DW", F32, 4096, 128, 256, "SGEMM_DMA_KT", "db", ws=2 * (128 * 256 + 128), splits=(2, 2)),
    case("dw_f32mfma_m1000", "DW", F32, 1000, 512, 512, "MGEMM_F32_DW", "db", relu=1),
    case("dw_f32mfma_m63_k96", "DW", F32, 63, 96, 96, "MGEMM_F32_DW", "db", relu=1),
    case("dw_f32mfma_m70000", "DW", F32, 70000, 128, 160, "MGEMM_F32_DW", "db", relu=1, splits=(35, 35)),
    case("dw_f32mfma_starved", "DW", F32, 5000, 128, 128, "MGEMM_F32_DW", "db", relu=1, ws=3 * (128 * 128 + 128), splits=(3, 3)),
    case("dw_f32mfma_offx", "DW", F32, 1024, 128, 128, "MGEMM_F32_DW", "db", offx=1),
    case("dw_head_k512", "DW", F32, 1000, 4, 512, "GRAD_W_HEAD", "db", relu=1),
    case("dw_head_k256_ldx", "DW", F32, 40000, 4, 256, "GRAD_W_HEAD", "db", relu=1, ldx=258),
    case("dw_fma_n32_k4", "DW", F32, 1000, 32, 4, "GRAD_W_F32", "db"),
    case("dw_fma_n4_ldg8", "DW", F32, 255, 4, 39, "GRAD_W_F32", "db", relu=1, ldg=8),
]
CASES_BY_NAME = {c["name"]: c for c in CASES}
assert len(CASES_BY_NAME) == len(CASES)

# Sibling pairs the code comments call bit-identical: the dispatcher is steered to each side by W16 present / absent, a leading
# dimension or a base offset only; the operands are the same values.
SIBLINGS = [
    # (name, case a, case b, outputs compared)
    ("hgemm_dma == mgemm_bf16 A16 (forward)",
     case("sib_fwd_hgemm", "FWD", T16, 1000, 512, 256, "HGEMM_DMA_M16", "X16", "W16", "b", "Mk16", "R", "Y16", relu=1, epi="LDS"),
     case("sib_fwd_mgemm", "FWD", T16, 1000, 512, 256, "MGEMM_BF16_A16_M16", "X16", "b", "Mk16", "R", "Y16", relu=1)),
    ("hgemm_dma == mgemm_bf16 A16 (dX)",
     case("sib_dx_hgemm", "DX", T16, 255, 512, 512, "HGEMM_DMA_M16", "X16", "W16", "Mk16", "Y16"),
     case("sib_dx_mgemm", "DX", T16, 255, 512, 512, "MGEMM_BF16_A16_M16", "X16", "Mk16", "Y16")),
    ("hgemm_dma_kt == mgemm_bf16 dW form",
     case("sib_dw_hkt", "DW", BF16, 4096, 512, 512, "HGEMM_DMA_KT", "X16", "G16", "db", relu=1),
     case("sib_dw_mgemm", "DW", BF16, 4096, 512, 512, "MGEMM_BF16_DW_A16B16", "X16", "G16", "db", relu=1, ldx=516)),
    ("LDS epilogue == register epilogue (fp32 DMA kernel)",
     case("sib_epi_lds", "FWD", F32, 1000, 160, 128, "SGEMM_DMA", "b", "Mk", "R", relu=1, epi="LDS"),
     case("sib_epi_reg", "FWD", F32, 1000, 160, 128, "SGEMM_DMA", "b", "Mk", "R", relu=1, ldy=161, epi="REG_ELEM")),
    ("LDS epilogue == register epilogue (bf16 DMA kernel, bf16 copy)",
     case("sib_epi16_lds", "FWD", T16, 255, 512, 256, "HGEMM_DMA_M16", "X16", "W16", "b", "Mk16", "R", "Y16", epi="LDS"),
     case("sib_epi16_reg", "FWD", T16, 255, 512, 256, "HGEMM_DMA_M16", "X16", "W16", "b", "Mk16", "R", "Y16", offy=2,
          epi="REG_ELEM")),
    ("k_head_dx == k_gemm_f32",
     case("sib_head_dx", "HEAD_DX", F32, 1000, 512, 4, "HEAD_DX", "Mk"),
     case("sib_head_fma", "DX", F32, 1000, 512, 4, "GEMM_F32", "Mk")),
]
SIBLING_CASES = [c for _, a, b in SIBLINGS for c in (a, b)]


def bf16_round(t):
    """Round-to-nearest-even to bf16, back as the input's dtype (what v_cvt_pk_bf16_f32 gives)."""
    return t.to(torch.bfloat16).to(t.dtype)


def gamma(n):
    return n * 2.0 ** -24


def reference(a, b, *, relu=False, bias=None, mk=None, mk16=None, r=None, acc0=None, x3=False):
    """fp64 value and elementwise bound of  C = mask(act(a) b^T + bias) + r  (+ acc0): a (M, K), b (N, K) — the exact operands
    the kernel multiplies (bf16-rounded already for the bf16 modes).  mk: fp32 mask (keeps > 0); mk16: bf16 bits as int16/int32
    (keeps sign clear and nonzero).  Returns (value, bound, keep)."""
    a64 = a.double()
    if relu:
        a64 = a64.clamp_min(0.0)
    b64 = b.double()
    v = a64 @ b64.T
    mag = a64.abs() @ b64.abs().T
    K = a.shape[1]
    if bias is not None:
        v = v + bias.double()
        mag = mag + bias.double().abs()
    keep = None
    if mk is not None:
        keep = mk.double() > 0
    if mk16 is not None:
        bits = mk16.to(torch.int32) & 0xFFFF
        keep = ((bits & 0x8000) == 0) & ((bits & 0x7FFF) != 0)
    if keep is not None:
        v = torch.where(keep, v, torch.zeros_like(v))
        mag = torch.where(keep, mag, torch.zeros_like(mag))
    extra = 0
    if r is not None:
        v = v + r.double()
        mag = mag + r.double().abs()
        extra = 1
    if acc0 is not None:
        v = v + acc0.double()
        mag = mag + acc0.double().abs()
        extra = 1
    bound = 2 * gamma(K + 2 + extra) * mag
    if x3:
        bound = bound + 2.0 ** -14 * (a64.abs() @ b64.abs().T)
    return v, bound, keep


def worst_ratio(y, v, bound):
    """max |y - v| / bound over the elements (inf where the bound is 0 and y differs; nan in y counts as inf)."""
    d = (y.double() - v).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    zero = bound == 0
    r = torch.where(zero, torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))), d / torch.where(zero, torch.ones_like(bound), bound))
    return float(r.max()) if r.numel() else 0.0
