"""FP8 (e4m3fn) path on the CPU: the torch formulas of ``ops.fp8`` (the reference semantics the HIP
kernels are tested against), the config key and the torch-emulated FP8 model."""

import pytest
import torch

from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
from distributed_llm_backend_benchmark_amd.ops import fp8, linear_fp8, quantize_rows
from distributed_llm_backend_benchmark_amd.parallel.comm import Comm
from distributed_llm_backend_benchmark_amd.utils.config import (DEFAULT_CONFIG, ConfigError,
                                                                validate_config)

E4M3 = torch.float8_e4m3fn


def _formula(x):
    """The issue's semantics, written out row by row."""
    xf = x.float()
    q = torch.zeros(xf.shape, dtype=E4M3)
    s = torch.ones(xf.shape[0], dtype=torch.float32)
    for i in range(xf.shape[0]):
        amax = xf[i].abs().max()
        if amax == 0:
            continue
        inv = torch.tensor(448.0, dtype=torch.float32) / amax
        s[i] = amax / torch.tensor(448.0, dtype=torch.float32)
        q[i] = (xf[i] * inv).to(E4M3)
    return q, s


def _rows():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(12, 256, generator=g).to(torch.bfloat16)
    x[3] = 0
    x[5, 17] = 3e38
    x[7] = 1e-30
    x[9] = -2.5
    return x


def _bits(q):
    return q.view(torch.uint8)


def test_quantize_rows_matches_formula_bitwise():
    x = _rows()
    q, s = quantize_rows(x)
    rq, rs = _formula(x)
    assert q.dtype == E4M3 and s.dtype == torch.float32 and s.shape == (12,)
    assert torch.equal(_bits(q), _bits(rq))
    assert torch.equal(s, rs)
    assert s[3] == 1 and not _bits(q)[3].any()
    assert not torch.isnan(q.float()).any() and q.float().abs().max() <= 448


def test_quantize_rows_strided_view_and_leading_dims():
    g = torch.Generator().manual_seed(1)
    big = torch.randn(64, 1536, generator=g).to(torch.bfloat16)
    x = big[:, :512]
    q, s = quantize_rows(x)
    rq, rs = _formula(x.contiguous())
    assert torch.equal(_bits(q), _bits(rq)) and torch.equal(s, rs)
    q3, s3 = quantize_rows(x.reshape(4, 16, 512))
    assert q3.shape == (4, 16, 512) and s3.shape == (4, 16)
    assert torch.equal(_bits(q3).reshape(64, 512), _bits(rq))


def test_dequantised_values_are_close():
    x = _rows()
    q, s = quantize_rows(x)
    xf = x.float()
    err = (q.float() * s[:, None] - xf).abs()
    # 3 mantissa bits (half an ulp = 2^-4 relative) plus the subnormal step of the scaled grid
    bound = 2.0 ** -4 * xf.abs() + s[:, None] * 2.0 ** -9
    assert (err <= bound).all()


@pytest.mark.parametrize("act", [None, "gelu", "gelu_tanh"])
def test_linear_fp8_cpu_equals_dequantised_product(act):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(24, 256, generator=g).to(torch.bfloat16)
    w = torch.randn(64, 256, generator=g).to(torch.bfloat16)
    bias = torch.randn(64, generator=g).to(torch.bfloat16)
    res = torch.randn(24, 64, generator=g).to(torch.bfloat16)
    xq, xs = quantize_rows(x)
    wq, ws = quantize_rows(w)
    ref = (xq.float() * xs[:, None]) @ (wq.float() * ws[:, None]).t() + bias.float()
    if act == "gelu":
        ref = torch.nn.functional.gelu(ref)
    elif act == "gelu_tanh":
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
    ref = ref + res.float()
    out = linear_fp8(xq, xs, wq, ws, bias=bias, act=act, residual=res, out_dtype=torch.float32)
    assert out.dtype == torch.float32
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-4)
    out16 = linear_fp8(xq, xs, wq, ws, bias=bias, act=act, residual=res)
    assert out16.dtype == torch.bfloat16
    torch.testing.assert_close(out16.float(), ref, rtol=2.0 ** -8, atol=1e-3)


@pytest.mark.parametrize("dist", ["gauss", "uniform"])
@pytest.mark.parametrize("K", [128, 512, 4096])
def test_end_to_end_error_is_fp8_sized(dist, K):
    """Relative Frobenius error of the quantised product against the fp32 product of the bf16
    inputs: 0.036-0.037 measured for per-row e4m3; below 0.05 (that plus a third, for bf16 output
    rounding and sample spread) and above 0.01 (a path that silently ran bf16 fails)."""
    g = torch.Generator().manual_seed(K)
    make = (lambda *s: torch.randn(*s, generator=g)) if dist == "gauss" else \
        (lambda *s: torch.rand(*s, generator=g) * 2 - 1)
    x = make(64, K).to(torch.bfloat16)
    w = make(128, K).to(torch.bfloat16)
    ref = x.float() @ w.float().t()
    out = fp8.fp8_linear(x, w).float()
    rel = ((out - ref).norm() / ref.norm()).item()
    print(f"fp8 end-to-end rel error {dist} K={K}: {rel:.4f}")
    assert 0.01 < rel < 0.05


def _cfg(**ex):
    cfg = {k: dict(v) for k, v in DEFAULT_CONFIG.items()}
    cfg["execution"].update(ex)
    return cfg


def test_config_gemm_dtype():
    assert validate_config(_cfg())["execution"]["gemm_dtype"] == "bf16"
    base = _cfg()
    del base["execution"]["gemm_dtype"]
    assert validate_config(base)["execution"]["gemm_dtype"] == "bf16"
    assert validate_config(_cfg(gemm_dtype="fp8"))["execution"]["gemm_dtype"] == "fp8"
    with pytest.raises(ConfigError, match="gemm_dtype"):
        validate_config(_cfg(gemm_dtype="int8"))
    bad = _cfg(gemm_dtype="fp8")
    bad["model"]["hidden_size"] = 320
    bad["parallelism"]["world_size"] = 1
    with pytest.raises(ConfigError, match="model.hidden_size"):
        validate_config(bad)
    bad["execution"]["gemm_dtype"] = "bf16"
    validate_config(bad)                      # the width rule binds only when fp8 is asked for
    ffn = _cfg(gemm_dtype="fp8")
    ffn["model"]["ffn_intermediate"] = 16384 + 256     # / 4 ranks = 4160, not a multiple of 128
    with pytest.raises(ConfigError, match="model.ffn_intermediate"):
        validate_config(ffn)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


def _model(gemm_dtype, seed=3):
    comm = Comm(0, 1, 0, "gloo", torch.device("cpu"))
    return LLM(hidden_size=256, num_layers=2, num_heads=4, ffn_intermediate=512, comm=comm,
               seed=seed, init_std=0.02, kernels="torch", gemm_dtype=gemm_dtype)


def test_llm_torch_fp8_differs_from_bf16_by_quantisation_noise():
    x = torch.randn(2, 16, 256, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    m16, m8 = _model("bf16"), _model("fp8")
    with torch.inference_mode():
        y16 = m16(x)
        y8 = m8(x)
    rel = _rel(y8, y16)
    print(f"LLM torch fp8 vs bf16 rel error: {rel:.4f}")
    assert y8.shape == y16.shape and torch.isfinite(y8.float()).all()
    assert 0.005 < rel < 0.2
    with pytest.raises(ValueError, match="gemm_dtype"):
        _model("int8")


def test_weight_cache_requantises_after_load_from_dense():
    x = torch.randn(1, 8, 256, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    a, b = _model("fp8", seed=6), _model("fp8", seed=7)
    w = a.layers[0].qkv_proj.weight
    with torch.no_grad():
        ya = a(x)
        wq0, ws0 = fp8.quantize_weight(w, "torch")
        assert fp8.quantize_weight(w, "torch")[0] is wq0          # cached
        yb = b(x)
        assert _rel(ya, yb) > 0.1                                 # different weights
        a.load_from_dense(b.state_dict())
        wq1, ws1 = fp8.quantize_weight(w, "torch")
        assert wq1 is not wq0
        rq, rs = quantize_rows(b.layers[0].qkv_proj.weight)
        assert torch.equal(_bits(wq1), _bits(rq)) and torch.equal(ws1, rs)
        assert torch.equal(a(x), yb)
