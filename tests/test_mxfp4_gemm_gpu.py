"""MXFP4 x MXFP4 GEMM and its row quantiser on the GPU (``csrc/gemm_mxfp4.hip``) against plain
fp64 torch: quantiser bits, exact products with a scale that differs per (row, k-block), random
operands, epilogues, refusals and the bf16-in / bf16-out ``mxfp4_linear``."""

import functools

import pytest
import torch

from distributed_llm_backend_benchmark_amd.ops import (dequantize_mxfp4, gemm, linear_mxfp4,
                                                       mxfp4, mxfp4_linear, quantize_rows_mxfp4)
from distributed_llm_backend_benchmark_amd.ops.fp8 import _epilogue_torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


def _quant_rows(M, K):
    """Random normal rows, then per row one special 32-block (the rest of the row stays random)."""
    g = torch.Generator(device=DEV).manual_seed(K + M)
    x = torch.randn(M, K, device=DEV, generator=g)
    ties = torch.tensor(TIES, device=DEV).repeat(5)[:32]
    i = torch.arange(32, device=DEV)
    sign = torch.where(i % 3 == 0, -1.0, 1.0)
    x[0, :32] = ties * sign * 4                      # amax 20 -> scale 4: every tie, both signs
    x[1, :32] = ties * sign * 2.0 ** -20
    x[2, :32] = torch.linspace(6.05, 7.9, 32, device=DEV) * sign     # (6, 8) after scaling by 1
    x[3, :32] = 0                                    # all-zero block
    x[4, :32] = torch.where(i == 5, 4.0, -0.01)      # amax 4: the rest rounds to -0
    x[5, :32] = sign * 2.0 ** -126                   # bottom clamp, b = 2
    x[5, 3] = 2.0 ** -130                            # bf16 subnormal
    x[6, :32] = sign * 3.0e38                        # near the largest finite bf16
    x[7, :32] = -0.0
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("shape", [(8, 32), (40, 128), (256, 512), (24, 4096), (8, 16384)])
def test_quantiser_bit_identical(shape):
    M, K = shape
    x = _quant_rows(M, K)
    rc, rs = mxfp4._quantize_rows(x.float())
    c, s = quantize_rows_mxfp4(x)
    assert c.shape == (M, K // 2) and s.shape == (M, K // 32)
    assert torch.equal(s, rs) and torch.equal(c, rc), (c != rc).nonzero()[:4].tolist()


def test_quantiser_strided_input_and_canary():
    lib = mxfp4._lib.lib()
    M, K = 64, 512
    big = torch.cat([_quant_rows(M, K), _quant_rows(M, 1024)], dim=1)      # ld 1536
    x = big[:, :K]
    rc, rs = mxfp4._quantize_rows(x.float())
    cbuf = torch.full((M + 2, K // 2 + 64), 0xAB, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((M + 2, K // 32 + 16), 0xCD, dtype=torch.uint8, device=DEV)
    rc_ = lib.dlbb_quant_mxfp4_rows(x.data_ptr(), x.stride(0), cbuf[1].data_ptr(), cbuf.stride(0),
                                    sbuf[1].data_ptr(), sbuf.stride(0), M, K,
                                    mxfp4._lib.stream(x.device))
    assert rc_ == 0
    assert torch.equal(cbuf[1:M + 1, :K // 2], rc) and torch.equal(sbuf[1:M + 1, :K // 32], rs)
    assert (cbuf[0] == 0xAB).all() and (cbuf[M + 1] == 0xAB).all() and (cbuf[:, K // 2:] == 0xAB).all()
    assert (sbuf[0] == 0xCD).all() and (sbuf[M + 1] == 0xCD).all() and (sbuf[:, K // 32:] == 0xCD).all()


@functools.lru_cache(maxsize=None)
def _exact_operands(M, N, K):
    """All 16 codes, asymmetric in A and B; scale bytes that differ over the 8 k-blocks of a
    K-tile; the fp64 product; sum|a||b| / q, q = the smallest product 0.25 * 2^(min exponents)."""
    m = torch.arange(M, device=DEV).view(M, 1)
    n = torch.arange(N, device=DEV).view(N, 1)
    k = torch.arange(K, device=DEV).view(1, K)
    kb = torch.arange(K // 32, device=DEV).view(1, K // 32)
    ca = (m * 7 + k * 3 + (m * k) % 5) % 16
    cb = (n * 5 + k * 11 + n // 3 + (n * k) % 7) % 16
    k8 = kb % 8                                            # k-block inside the K-tile
    # for any two k-blocks of a K-tile some row has different scales in them, in A and in B
    sa = (127 + (kb * 3 + m) % 4 + k8 // 4).to(torch.uint8)               # exponents 0..4
    sb = (127 - (k8 + 2 * n) % 3 - torch.where(n % 2 == 0, k8 // 4, k8 % 2)).to(torch.uint8)  # -3..0
    pack = lambda c: (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8).contiguous()
    a, b = pack(ca), pack(cb)
    ad, bd = dequantize_mxfp4(a, sa).double(), dequantize_mxfp4(b, sb).double()
    return a, sa, b, sb, ad @ bd.t(), (ad.abs() @ bd.abs().t()) * 32


# smallest legal; one K-tile; three K-tiles (buffer parity); tile map; ragged M, N; balanced issue
EXACT_SHAPES = [(8, 64, 256), (256, 256, 256), (256, 256, 768), (512, 512, 1024),
                (264, 320, 512), (256, 256, 8192)]


@pytest.mark.parametrize("shape", EXACT_SHAPES)
def test_exact_products_with_block_scales(shape):
    M, N, K = shape
    a, sa, b, sb, ref, units = _exact_operands(M, N, K)
    assert len(set(sa[1, :8].tolist())) > 1 and len(set(sb[1, :8].tolist())) > 1
    assert units.max() < 2 ** 24          # every partial sum, in any order, is exact in fp32
    out = linear_mxfp4(a, sa, b, sb, out_dtype=torch.float32)
    assert out.dtype == torch.float32 and out.shape == (M, N)
    assert torch.equal(out.double(), ref), (out.double() != ref).nonzero()[:4].tolist()
    out16 = linear_mxfp4(a, sa, b, sb, out_dtype=torch.bfloat16)
    assert torch.equal(out16, ref.to(torch.bfloat16))


@functools.lru_cache(maxsize=None)
def _random_operands(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    r = lambda rows, cols, lo, hi: torch.randint(lo, hi, (rows, cols), dtype=torch.uint8,
                                                 device=DEV, generator=g)
    a, b = r(M, K // 2, 0, 256), r(N, K // 2, 0, 256)
    sa, sb = r(M, K // 32, 120, 135), r(N, K // 32, 120, 135)
    ad, bd = dequantize_mxfp4(a, sa).double(), dequantize_mxfp4(b, sb).double()
    return a, sa, b, sb, ad @ bd.t(), ad.abs() @ bd.abs().t()


@pytest.mark.parametrize("shape", [(256, 256, 4096), (520, 384, 1024)])
def test_random_codes_and_scales(shape):
    """fp32 sums in any order: (K + 8) 2^-24 sum|a||b|; bf16 output adds 2^-8 |ref|."""
    M, N, K = shape
    a, sa, b, sb, ref, mag = _random_operands(M, N, K)
    bound = (K + 8) * 2.0 ** -24 * mag
    out = linear_mxfp4(a, sa, b, sb, out_dtype=torch.float32)
    assert ((out.double() - ref).abs() <= bound).all()
    out16 = linear_mxfp4(a, sa, b, sb, out_dtype=torch.bfloat16)
    assert ((out16.double() - ref).abs() <= bound + 2.0 ** -8 * ref.abs()).all()


@functools.lru_cache(maxsize=None)
def _epilogue_operands():
    M, N, K = 264, 320, 512
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) * 0.05
    xc, xs = mxfp4._quantize_rows(x)
    wc, ws = mxfp4._quantize_rows(w)
    bias = torch.randn(N, device=DEV, generator=g).to(torch.bfloat16)
    res = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    prod = dequantize_mxfp4(xc, xs).double() @ dequantize_mxfp4(wc, ws).double().t()
    return xc, xs, wc, ws, bias, res, prod


EPILOGUES = {"bias": dict(bias=True), "gelu_erf": dict(act="gelu"),
             "gelu_tanh": dict(act="gelu_tanh"), "residual": dict(residual=True),
             "all": dict(bias=True, act="gelu", residual=True),
             "all_tanh": dict(bias=True, act="gelu_tanh", residual=True)}


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", list(EPILOGUES))
def test_epilogues(case, out_dtype):
    xc, xs, wc, ws, bias, res, prod = _epilogue_operands()
    c = EPILOGUES[case]
    kw = dict(bias=bias if c.get("bias") else None, act=c.get("act"),
              residual=res if c.get("residual") else None)
    ref = _epilogue_torch(prod, kw["bias"], kw["act"], kw["residual"], torch.float64)
    out = linear_mxfp4(xc, xs, wc, ws, out_dtype=out_dtype, **kw)
    assert out.dtype == out_dtype
    assert float((out.double() - ref).abs().max() / ref.abs().max()) < 1e-2


def _zeros(M, N, K):
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)
    return z(M, K // 2), z(M, K // 32) + 127, z(N, K // 2), z(N, K // 32) + 127


@pytest.mark.parametrize("case", ["K%256", "M%8", "N%64", "misaligned", "scales"])
def test_contract_violations_raise_and_launch_nothing(case):
    calls = dict(mxfp4.CALLS)
    M, N, K = {"K%256": (64, 64, 384), "M%8": (12, 64, 256), "N%64": (64, 96, 256)}.get(
        case, (64, 64, 256))
    xc, xs, wc, ws = _zeros(M, N, K)
    if case == "misaligned":
        raw = torch.zeros(M * K // 2 + 16, dtype=torch.uint8, device=DEV)
        xc = raw[1:1 + M * K // 2].view(M, K // 2)
        assert xc.data_ptr() % 16 == 1
    if case == "scales":
        xs = torch.full((M, K // 32 + 1), 127, dtype=torch.uint8, device=DEV)
    out = torch.full((M, N), 5.0, device=DEV)
    with pytest.raises(ValueError):
        linear_mxfp4(xc, xs, wc, ws, out_dtype=torch.float32, out=out)
    if case in ("K%256", "M%8", "N%64"):
        with pytest.raises(ValueError):              # the wrapper refuses before quantising
            mxfp4_linear(torch.zeros(M, K, device=DEV, dtype=torch.bfloat16),
                         torch.zeros(N, K, device=DEV, dtype=torch.bfloat16))
    torch.cuda.synchronize()
    assert (out == 5.0).all() and dict(mxfp4.CALLS) == calls


def test_mxfp4_linear_quantises_and_counts_launches():
    """bf16 in, bf16 out: the activation through the HIP quantiser, the weight through the cache
    of ``w4_linear``; equal to the GEMM on the torch-quantised operands, one counted launch."""
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn(2, 32, 512, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(192, 512, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    before = gemm.kernel_mix()["mxfp4"]["calls"]
    y = mxfp4_linear(x, w, act="gelu")
    assert gemm.kernel_mix()["mxfp4"]["calls"] == before + 1
    assert [64, 192, 512] in gemm.kernel_mix()["mxfp4"]["shapes"]
    xc, xs = mxfp4._quantize_rows(x.reshape(64, 512).float())
    wc, ws = mxfp4.quantize_weight_mxfp4(w)
    ref = _epilogue_torch(dequantize_mxfp4(xc, xs).double() @ dequantize_mxfp4(wc, ws).double().t(),
                          None, "gelu", None, torch.float64)
    assert y.dtype == torch.bfloat16 and y.shape == (2, 32, 192)
    assert ((y.double().reshape(64, 192) - ref).abs() <= 2.0 ** -7 * ref.abs() + 1e-3).all()
