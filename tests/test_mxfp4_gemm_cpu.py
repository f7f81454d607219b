"""CPU side of the MXFP4 GEMM path: the torch form of ``linear_mxfp4`` against fp64 and the
shape check of the TP widths."""

import os

import pytest
import torch
import yaml

from distributed_llm_backend_benchmark_amd.ops import (dequantize_mxfp4, linear_mxfp4,
                                                       quantize_rows_mxfp4)
from distributed_llm_backend_benchmark_amd.utils.config import (ConfigError,
                                                                check_mxfp4_gemm_shapes)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_linear_mxfp4_torch_path_against_fp64(out_dtype):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 12, 64, generator=g).to(torch.bfloat16)
    w = torch.randn(40, 64, generator=g).to(torch.bfloat16)
    bias = torch.randn(40, generator=g).to(torch.bfloat16)
    xc, xs = quantize_rows_mxfp4(x)
    wc, ws = quantize_rows_mxfp4(w)
    assert xc.shape == (2, 12, 32) and xs.shape == (2, 12, 2)
    ref = dequantize_mxfp4(xc.reshape(24, 32), xs.reshape(24, 2)).double() \
        @ dequantize_mxfp4(wc, ws).double().t() + bias.double()
    out = linear_mxfp4(xc, xs, wc, ws, bias=bias, out_dtype=out_dtype)
    assert out.dtype == out_dtype and out.shape == (2, 12, 40)
    tol = 2.0 ** -20 if out_dtype == torch.float32 else 2.0 ** -8
    assert ((out.double().reshape(24, 40) - ref).abs() <= tol * ref.abs() + 1e-6).all()
    with pytest.raises(ValueError):
        linear_mxfp4(xc, xs[..., :1], wc, ws)


def test_check_mxfp4_gemm_shapes():
    c7 = yaml.safe_load(open(os.path.join(REPO, "config", "7b_config.yaml")))
    c13 = yaml.safe_load(open(os.path.join(REPO, "config", "13b_config.yaml")))
    check_mxfp4_gemm_shapes(c7, 8)
    with pytest.raises(ConfigError, match="640"):
        check_mxfp4_gemm_shapes(c13, 8)
