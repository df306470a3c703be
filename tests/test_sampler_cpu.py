"""The host model of the samplers (tests/sampler_util.py) pinned on the CPU: published Philox4x32-10 vectors, an independent
implementation of the rounds, the draw layout written out a second time from include/pnr.h, and the accounting of the
resampling test run against the fp32 oracle, so that tests/test_gpu_sampler.py compares the kernels with a checked model."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import sampler_util as su
from oracle import pixelnerf_oracle as orc

SEEDS = [0, 1234, 2 ** 63 + 5, 2 ** 64 - 1]
BASES = [0, 7, 2 ** 32 - 3, 2 ** 40 + 1]

# Random123 kat_vectors, philox4x32-10: counter, key, result
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        got = su.philox4x32_10(key[0], key[1], *ctr)
        assert tuple(int(x) for x in got) == want, [hex(int(x)) for x in got]
    # the three at once: the vectorised form
    got = su.philox4x32_10(*[np.array(c, dtype=np.uint64) for c in zip(*[k + c for c, k, _ in KAT])])
    assert [tuple(int(g[i]) for g in got) for i in range(3)] == [w for _, _, w in KAT]


_ATEN_SRC = r"""
#include <ATen/core/PhiloxRNGEngine.h>
#include <cstdio>
int main() {
    unsigned long long k, off, sub;
    while (std::scanf("%llu %llu %llu", &k, &off, &sub) == 3) {
        at::philox_engine e(k, sub, off);       // key = seed, counter = (offset lo, offset hi, subsequence lo, subsequence hi)
        unsigned a = e(), b = e(), c = e(), d = e();
        std::printf("%u %u %u %u\n", a, b, c, d);
    }
    return 0;
}
"""
_ROCRAND_SRC = r"""
#include <hip/hip_runtime.h>
#include <rocrand/rocrand_philox4x32_10.h>
#include <cstdio>
int main() {
    unsigned long long k, off, sub;
    while (std::scanf("%llu %llu %llu", &k, &off, &sub) == 3) {
        rocrand_device::philox4x32_10_engine e(k, sub, off * 4ULL);      // its offset counts 32-bit words
        uint4 v = e.next4();
        std::printf("%u %u %u %u\n", v.x, v.y, v.z, v.w);
    }
    return 0;
}
"""


def _build_cross_check(tmp):
    """Stand-alone host program around an independent Philox: torch's ATen header, else rocRAND's; (exe, offset bits)."""
    tried = []
    inc = os.path.join(os.path.dirname(torch.__file__), "include")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx and os.path.exists(os.path.join(inc, "ATen", "core", "PhiloxRNGEngine.h")):
        src, exe = os.path.join(tmp, "aten_philox.cpp"), os.path.join(tmp, "aten_philox")
        with open(src, "w") as f:
            f.write(_ATEN_SRC)
        p = subprocess.run([cxx, "-std=c++17", "-O1", "-I", inc, src, "-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            return exe, 64, "ATen/core/PhiloxRNGEngine.h"
        tried.append("ATen: " + p.stderr.strip()[-300:])
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc) and os.path.exists("/opt/rocm/include/rocrand/rocrand_philox4x32_10.h"):
        src, exe = os.path.join(tmp, "rocrand_philox.hip"), os.path.join(tmp, "rocrand_philox")
        with open(src, "w") as f:
            f.write(_ROCRAND_SRC)
        p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", src, "-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            return exe, 62, "rocrand_philox4x32_10.h"
        tried.append("rocRAND: " + p.stderr.strip()[-300:])
    pytest.skip("no independent Philox header compiles for the host here: " + " | ".join(tried))


def test_philox_against_an_independent_header(tmp_path):
    exe, off_bits, which = _build_cross_check(str(tmp_path))
    rng = np.random.default_rng(7)
    n = 300
    key = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    off = rng.integers(0, 2 ** off_bits, n, dtype=np.uint64)
    sub = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    key[:2], off[:2], sub[:2] = (0, 2 ** 64 - 1), (0, 2 ** off_bits - 1), (0, 2 ** 64 - 1)
    text = "".join(f"{int(k)} {int(o)} {int(s)}\n" for k, o, s in zip(key, off, sub))
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    theirs = np.array([[int(x) for x in ln.split()] for ln in p.stdout.splitlines()], dtype=np.uint64)
    assert theirs.shape == (n, 4), which
    m, s = su.MASK, su.S32
    ours = np.stack(su.philox4x32_10(key & m, key >> s, off & m, off >> s, sub & m, sub >> s), -1)
    assert np.array_equal(ours, theirs), which


def _layout_again(seed, ray, kind, idx):
    """The draw layout a second time, from include/pnr.h's words: the word a draw is made of."""
    ident = {"noise_c": 0, "u": 1, "r": 2, "g": 3}[kind]
    ray = ray % 2 ** 64
    blk = idx if kind == "g" else idx // 4
    return su.philox4x32_10(seed % 2 ** 32, seed // 2 ** 32, ray % 2 ** 32, ray // 2 ** 32, ident, blk)


def test_draw_layout_matches_its_definition():
    for seed, base in itertools.product(SEEDS, BASES):
        rays = su.global_ray(base, 5)
        assert [int(x) for x in rays] == [base + i for i in range(5)]
        for kind in ("noise_c", "u", "r"):
            got = su.draws(seed, rays, kind, 11)
            assert got.dtype == np.float32 and got.shape == (5, 11)
            for i, j in itertools.product(range(5), (0, 1, 3, 4, 5, 7, 8, 10)):
                word = int(_layout_again(seed, base + i, kind, j)[j % 4])
                assert float(got[i, j]) == (word >> 8) / 2.0 ** 24, (seed, base, kind, i, j)
        g = su.draws(seed, rays, "g", 6)
        for i, j in itertools.product(range(5), range(6)):
            w = _layout_again(seed, base + i, "g", j)
            a = np.float32(1.0) - np.float32((int(w[0]) >> 8) / 2.0 ** 24)
            arg = np.float32(6.28318530717958647692) * np.float32((int(w[1]) >> 8) / 2.0 ** 24)
            assert type(arg) is np.float32 and 0 < a <= 1
            assert g[i, j] == np.sqrt(-2.0 * np.log(np.float64(a))) * np.cos(np.float64(arg)), (seed, base, i, j)


def test_global_ray_formula():
    B = 6
    assert su.global_ray(3, 2 * B, B, 0).tolist() == list(range(3, 3 + 2 * B))
    assert su.global_ray(3, 2 * B, B, 2 * B).tolist() == [3 + i for i in range(B)] + [3 + 2 * B + i for i in range(B)]
    assert su.global_ray(2 ** 40, 2, 1, 5).tolist() == [2 ** 40, 2 ** 40 + 5]


def test_no_two_draws_of_a_ray_share_a_word():
    for seed, ray in itertools.product(SEEDS, (0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 1)):
        seen = {}
        for kind in ("noise_c", "u", "r", "g"):
            for idx in range(140):
                k = su.counter_of(seed, ray, kind, idx)
                words = [(k[2:6], 0), (k[2:6], 1)] if kind == "g" else [(k[2:6], k[6])]
                for wd in words:
                    assert wd not in seen, (kind, idx, seen[wd])
                    seen[wd] = (kind, idx)
                assert k[:2] == (seed & 0xFFFFFFFF, seed >> 32) and k[2] + (k[3] << 32) == ray
                assert k[4:] == tuple(int(x) for x in (su.DRAW_ID[kind], idx if kind == "g" else idx >> 2, 0 if kind == "g" else idx & 3))
    # and the streams really differ: different draw ids, the tail quad, the ray's high word
    rays = np.arange(40, dtype=np.int64)
    d = {k: su.draws(1234, rays, k, 13) for k in ("noise_c", "u", "r")}
    for a, b in itertools.combinations(d, 2):
        assert (d[a] != d[b]).mean() > 0.99, (a, b)
    assert len(np.unique(d["u"])) > 0.99 * d["u"].size                  # idx 4..7 are not idx 0..3 again
    for kind in ("noise_c", "u", "r", "g"):
        lo, hi = su.draws(1234, rays, kind, 13), su.draws(1234, rays + 2 ** 32, kind, 13)
        assert (lo != hi).mean() > 0.99, kind
    u = su.draws(99, np.arange(4096), "u", 16).astype(np.float64)
    assert abs(u.mean() - 0.5) < 5e-3 and abs(u.var() - 1 / 12) < 5e-3 and u.min() >= 0 and u.max() < 1
    g = su.draws(99, np.arange(4096), "g", 16)
    assert abs(g.mean()) < 2e-2 and abs(g.var() - 1) < 3e-2


# --------------------------------------------------------------------------------------- accounting self-test
def oracle_rows(case, u, r, std):
    """sample_fine + sample_fine_depth + cat + sort of the fp32 oracle."""
    t = torch.from_numpy
    rays, parts = t(case["rays"]), [t(case["zc"])]
    if case["n_imp"]:
        parts.append(orc.sample_fine(rays, t(case["w"]), case["Kc"], case["lindisp"], t(np.ascontiguousarray(u)), t(np.ascontiguousarray(r))))
    if case["n_dep"]:
        parts.append(orc.sample_fine_depth(rays, t(case["depth"]), std, t(case["g"])))
    return torch.sort(torch.cat(parts, -1), -1)[0].numpy()


def run_all(rows_of):
    """check_rows over every shape, pair of bounds, lindisp, std and both runs; the summed statistics."""
    tot = {}
    for (Kc, n_imp, n_dep), (near, far), lindisp in itertools.product(su.SHAPES, su.BOUNDS, (False, True)):
        case = su.make_case(Kc, n_imp, n_dep, near, far, lindisp)
        for std in (case["stds"] if n_dep else case["stds"][:1]):
            for tagged, u, r in ((True, case["u"], case["r_tag"]), (False, case["u_rand"], case["r_rand"])):
                st = su.check_rows(case, rows_of(case, u, r, std), u, r, std, tagged)
                for k, v in st.items():
                    key = (k, tagged, Kc <= 300)
                    tot[key] = max(tot.get(key, 0), v) if k == "worst" else tot.get(key, 0) + v
    return tot


def test_accounting_against_the_fp32_oracle():
    """Every weight and draw family of the GPU test, with the fp32 oracle in the kernel's place: every draw's bin inside
    [lo, hi], the planted bins recovered, positions within the z tolerance — and the check is not vacuous.  Measured here
    (random-weight rays, random u): 0.040 % of the draws have lo < hi for Kc <= 300 (6.6 % for Kc >= 2048, where the margin
    is 141 * 2^-24 against bins of 2.5e-4); 91.7 % of the random-weight rays have lo == hi for every draw; the oracle's worst
    position error is 0.25 of the tolerance."""
    tot = run_all(oracle_rows)
    small = tot[("rand_ambiguous", False, True)] / tot[("rand_draws", False, True)]
    large = tot[("rand_ambiguous", False, False)] / max(tot[("rand_draws", False, False)], 1)
    clean = (tot[("rand_clean", False, True)] + tot[("rand_clean", False, False)]) / (tot[("rand_rays", False, True)] + tot[("rand_rays", False, False)])
    print(f"draws with lo < hi, random weights and u: Kc <= 300 {100 * small:.3f} %, larger {100 * large:.2f} %; "
          f"random-weight rays with lo == hi throughout {100 * clean:.1f} %; planted top-bin draws "
          f"{tot[('top_bin', True, True)] + tot[('top_bin', True, False)]}; worst |dz| / tol "
          f"{max(v for k, v in tot.items() if k[0] == 'worst'):.3f}")
    assert small <= 0.005
    assert clean >= 0.9
    assert tot[("top_bin", True, True)] > 0          # the unclamped top bin is among the planted draws


def test_accounting_notices_an_off_by_one_bin():
    case = su.make_case(64, 65, 0, 1.25, 2.75, False)
    rows = oracle_rows(case, case["u"], case["r_tag"], 0.0)
    su.check_rows(case, rows, case["u"], case["r_tag"], 0.0, True)
    t = torch.from_numpy
    shifted = orc.sample_fine(t(case["rays"]), t(case["w"]), 64, False, t(case["u"]), t(case["r_tag"]) + 1.0)       # every bin + 1
    bad = torch.sort(torch.cat([t(case["zc"]), shifted], -1), -1)[0].numpy()
    with pytest.raises(AssertionError):
        su.check_rows(case, bad, case["u"], case["r_tag"], 0.0, True)
    lost = rows[3].copy()
    k = int(np.nonzero(lost == case["zc"][3][20])[0][0])
    lost[k] = np.nextafter(lost[k], np.float32(0))                 # a coarse value off by one ulp: the row is no permutation
    with pytest.raises(su.Accounting):
        su.remove_coarse(np.sort(lost), case["zc"][3])
