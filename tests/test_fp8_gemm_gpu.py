"""FP8 (e4m3fn) kernels on the GPU (``csrc/gemm_fp8.hip``): the block-scaled-MFMA NT GEMM against
exact integer products and fp64 references, the one-pass row quantiser against the torch formula
bit for bit, the contract checks, the FP8 model against its torch emulation, and ``run_tp
--gemm-dtype fp8``."""

import functools
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_llm_backend_benchmark_amd.ops import fp8, gemm, linear_fp8, quantize_rows

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3 = torch.float8_e4m3fn
DEV = "cuda"


def _bits(q):
    return q.view(torch.uint8)


@functools.lru_cache(maxsize=None)
def _int_operands(M, N, K):
    """Integers in [-3, 4] (exact in e4m3): A differs per row and per k, B is asymmetric in
    (n, k) and unrelated to A; with the exact fp64 product."""
    m = torch.arange(M, device=DEV).view(M, 1)
    n = torch.arange(N, device=DEV).view(N, 1)
    k = torch.arange(K, device=DEV).view(1, K)
    a = ((m * 7 + k * 3 + (m * k) % 5) % 8 - 3).float()
    b = ((n * 5 + k * 11 + (n // 3) + (n * k) % 7) % 8 - 3).float()
    ref = a.double() @ b.double().t()
    return a.to(E4M3), b.to(E4M3), ref


INT_SHAPES = [(256, 256, 128),      # one K-tile
              (256, 256, 384),      # odd tile count (buffer parity)
              (512, 512, 1024),     # four workgroups: the workgroup -> tile map
              (264, 320, 256),      # ragged M and N inside the contract
              (8, 64, 128)]         # the smallest legal shape


@pytest.mark.parametrize("shape", INT_SHAPES)
def test_exact_integer_products(shape):
    M, N, K = shape
    a, b, ref = _int_operands(M, N, K)
    assert ref.abs().max() < 2 ** 24                     # every partial sum is exact in fp32
    one_m = torch.ones(M, device=DEV)
    one_n = torch.ones(N, device=DEV)
    out = linear_fp8(a, one_m, b, one_n, out_dtype=torch.float32)
    assert out.dtype == torch.float32 and out.shape == (M, N)
    bad = (out.double() != ref).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong elements, first {bad[:4].tolist()}"
    out16 = linear_fp8(a, one_m, b, one_n, out_dtype=torch.bfloat16)
    assert torch.equal(out16, ref.to(torch.bfloat16))


def test_row_and_column_scales_are_not_swapped():
    M, N, K = 256, 320, 256
    a, b, ref = _int_operands(M, N, K)
    m = torch.arange(M, device=DEV)
    n = torch.arange(N, device=DEV)
    sa = torch.pow(2.0, (m % 5 - 2).float()) * (1 + 2 * (m % 4)).float()        # 2^e x 1, 3, 5, 7
    sb = torch.pow(2.0, (n % 3).float()) * (1 + 2 * ((n // 3) % 3)).float()    # 2^e x 1, 3, 5
    want = ref * sa.double()[:, None] * sb.double()[None, :]
    out = linear_fp8(a, sa, b, sb, out_dtype=torch.float32)
    err = (out.double() - want).abs()
    assert (err <= 2.0 ** -22 * want.abs()).all(), float((err / want.abs().clamp_min(1e-30)).max())


@functools.lru_cache(maxsize=None)
def _random_operands(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M + N + K)

    def e4m3(rows):
        raw = torch.randint(0, 256, (rows, K), dtype=torch.uint8, device=DEV, generator=g)
        raw = torch.where((raw & 0x7F) == 0x7F, raw & 0xF0, raw)       # no NaN encodings
        return raw.view(E4M3)

    a, b = e4m3(M), e4m3(N)
    sa = torch.rand(M, device=DEV, generator=g) * 2 + 0.25
    sb = torch.rand(N, device=DEV, generator=g) * 2 + 0.25
    ad, bd = a.double(), b.double()
    scale = sa.double()[:, None] * sb.double()[None, :]
    return a, b, sa, sb, (ad @ bd.t()) * scale, (ad.abs() @ bd.abs().t()) * scale


@pytest.mark.parametrize("shape", [(256, 256, 4096), (520, 384, 1024)])
def test_random_e4m3_operands_and_scales(shape):
    """fp32 accumulation in any order: |out - ref| <= (K + 8) 2^-24 sum|a||b| sa sb; bf16 output
    adds its rounding, 2^-8 |ref|."""
    M, N, K = shape
    a, b, sa, sb, ref, mag = _random_operands(M, N, K)
    bound = (K + 8) * 2.0 ** -24 * mag
    out = linear_fp8(a, sa, b, sb, out_dtype=torch.float32)
    err = (out.double() - ref).abs()
    print(f"fp32 out {shape}: max err / bound = {float((err / bound).max()):.4f}")
    assert (err <= bound).all()
    out16 = linear_fp8(a, sa, b, sb, out_dtype=torch.bfloat16)
    err16 = (out16.double() - ref).abs()
    assert (err16 <= bound + 2.0 ** -8 * ref.abs()).all()


@functools.lru_cache(maxsize=None)
def _epilogue_operands():
    M, N, K = 264, 320, 512
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    xq, xs = quantize_rows(x, kernels="torch")
    wq, ws = quantize_rows(w, kernels="torch")
    bias = torch.randn(N, device=DEV, generator=g).to(torch.bfloat16)
    res = torch.randn(M, N, device=DEV, generator=g).to(torch.bfloat16)
    return xq, xs, wq, ws, bias, res


EPILOGUES = {"bias": dict(bias=True), "gelu_erf": dict(act="gelu"),
             "gelu_tanh": dict(act="gelu_tanh"), "residual": dict(residual=True),
             "all": dict(bias=True, act="gelu", residual=True),
             "all_tanh": dict(bias=True, act="gelu_tanh", residual=True)}


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", list(EPILOGUES))
def test_epilogues(case, out_dtype):
    xq, xs, wq, ws, bias, res = _epilogue_operands()
    c = EPILOGUES[case]
    kw = dict(bias=bias if c.get("bias") else None, act=c.get("act"),
              residual=res if c.get("residual") else None)
    ref = linear_fp8(xq, xs, wq, ws, out_dtype=torch.float32, kernels="torch", **kw)
    out = linear_fp8(xq, xs, wq, ws, out_dtype=out_dtype, **kw)
    assert out.dtype == out_dtype
    rel = float((out.float() - ref).abs().max() / ref.abs().max())
    print(f"epilogue {case} {out_dtype}: max|err| / max|ref| = {rel:.2e}")
    assert rel < 1e-2


def _special_rows(M, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g).to(torch.bfloat16)
    if M >= 8:
        x[1] = 0
        x[2, K // 3] = 3e38
        x[3] = 1e-30
        x[4] = -2.5
    return x


@pytest.mark.parametrize("shape", [(256, 512), (40, 128), (8, 16384), (24, 4096), (24, 8192),
                                   (16, 1024), (16, 2048), (10, 72)])
def test_quantiser_bit_identical_to_torch_formula(shape):
    M, K = shape
    x = _special_rows(M, K, K)
    rq, rs = quantize_rows(x, kernels="torch")           # the formula, on the same device
    q, s = quantize_rows(x)
    torch.cuda.synchronize()
    assert q.dtype == E4M3 and q.shape == (M, K) and s.shape == (M,)
    assert torch.equal(s, rs)
    bad = (_bits(q) != _bits(rq)).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} bytes differ, first {bad[:4].tolist()}"
    assert not torch.isnan(q.float()).any()


def test_quantiser_strided_input_and_canary():
    g = torch.Generator(device=DEV).manual_seed(11)
    big = torch.randn(64, 1536, device=DEV, generator=g).to(torch.bfloat16)
    x = big[:, :512]                                     # the "first H/P columns" view, ld 1536
    rq, rs = quantize_rows(x.contiguous(), kernels="torch")
    M, K = x.shape
    qbuf = torch.full((M + 2, K + 64), 0xAB, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((M + 2,), -7.0, device=DEV)
    q, s = quantize_rows(x, out_q=qbuf[1:M + 1, :K].view(E4M3), out_scale=sbuf[1:M + 1])
    torch.cuda.synchronize()
    assert torch.equal(_bits(q), _bits(rq)) and torch.equal(s, rs)
    assert torch.equal(qbuf[1:M + 1, :K], _bits(rq))
    assert (qbuf[0] == 0xAB).all() and (qbuf[M + 1] == 0xAB).all() and (qbuf[:, K:] == 0xAB).all()
    assert sbuf[0] == -7.0 and sbuf[M + 1] == -7.0
    q3, s3 = quantize_rows(big.view(4, 16, 1536)[..., :512])       # 3-D strided view, no copy
    assert q3.shape == (4, 16, 512) and torch.equal(_bits(q3).view(M, K), _bits(rq))
    assert torch.equal(s3.view(M), rs)


def test_contract_violations_raise_and_launch_nothing():
    calls = dict(fp8.CALLS)

    def operands(M, N, K):
        return (torch.zeros(M, K, device=DEV).to(E4M3), torch.ones(M, device=DEV),
                torch.zeros(N, K, device=DEV).to(E4M3), torch.ones(N, device=DEV))

    for M, N, K in ((64, 64, 192), (64, 96, 128), (12, 64, 128)):
        xq, xs, wq, ws = operands(M, N, K)
        out = torch.full((M, N), 5.0, device=DEV)
        with pytest.raises(ValueError):
            linear_fp8(xq, xs, wq, ws, out_dtype=torch.float32, out=out)
        torch.cuda.synchronize()
        assert (out == 5.0).all()
        with pytest.raises(ValueError):                  # the wrapper refuses before quantising
            fp8.fp8_linear(torch.zeros(M, K, device=DEV, dtype=torch.bfloat16),
                           torch.zeros(N, K, device=DEV, dtype=torch.bfloat16))
    M, N, K = 64, 64, 128
    xq, xs, wq, ws = operands(M, N, K)
    raw = torch.zeros(M * K + 16, dtype=torch.uint8, device=DEV)
    misaligned = raw[1:1 + M * K].view(M, K).view(E4M3)
    assert misaligned.data_ptr() % 16 == 1
    out = torch.full((M, N), 5.0, device=DEV)
    with pytest.raises(ValueError):
        linear_fp8(misaligned, xs, wq, ws, out_dtype=torch.float32, out=out)
    with pytest.raises(ValueError):
        linear_fp8(xq, xs, wq, ws, out_dtype=torch.float32, out=out, act="relu")
    with pytest.raises(ValueError):
        quantize_rows(torch.zeros(8, 16384 + 8, device=DEV, dtype=torch.bfloat16))
    torch.cuda.synchronize()
    assert (out == 5.0).all()
    assert dict(fp8.CALLS) == calls


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def test_model_fp8_hip_matches_torch_emulation():
    from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
    from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

    dev = torch.device("cuda", torch.cuda.current_device())

    def model(kernels, gemm_dtype):
        return LLM(hidden_size=512, num_layers=2, num_heads=4, ffn_intermediate=2048,
                   comm=Comm(0, 1, 0, "gloo", dev), seed=5, init_std=0.02, kernels=kernels,
                   gemm_dtype=gemm_dtype)

    x = torch.randn(2, 128, 512, device=dev,
                    generator=torch.Generator(device=dev).manual_seed(9)).to(torch.bfloat16)
    hip8, torch8, torch16 = model("hip", "fp8"), model("torch", "fp8"), model("torch", "bf16")
    assert torch.equal(hip8.layers[1].ffn_down.weight, torch16.layers[1].ffn_down.weight)
    before = gemm.kernel_mix()["fp8"]["calls"]
    with torch.no_grad():
        y_hip8 = hip8(x)
        calls = gemm.kernel_mix()["fp8"]["calls"] - before
        y_t8 = torch8(x)
        y_t16 = torch16(x)
    quant = _rel(y_t8, y_t16)
    impl = _rel(y_hip8, y_t8)
    total = _rel(y_hip8, y_t16)
    print(f"model: rel(hip_fp8, torch_fp8) = {impl:.4f}, rel(torch_fp8, torch_bf16) = {quant:.4f}, "
          f"rel(hip_fp8, torch_bf16) = {total:.4f}")
    assert torch.isfinite(y_hip8.float()).all()
    assert impl <= quant                 # implementation noise below quantisation noise
    assert total <= 1.25 * quant
    assert calls == 8                    # four linears x two layers
    mix = gemm.kernel_mix()["fp8"]
    assert [256, 1536, 512] in mix["shapes"] and [256, 512, 2048] in mix["shapes"]


def test_run_tp_gemm_dtype_fp8(tmp_path):
    """run_tp --shard-as 4 --gemm-dtype fp8: rank 0's shard of a 4-way FP8 TP forward under
    HIP-graph replay; the record goes to <backend>_<name>_shard4_fp8.json."""
    import yaml

    cfg = yaml.safe_load(open(os.path.join(REPO, "config", "1b_config.yaml")))
    cfg["model"]["num_layers"] = 2
    cfg["experiment"]["output_dir"] = str(tmp_path)
    cfg["execution"]["warmup_iterations"] = 2
    cfg["execution"]["benchmark_iterations"] = 3
    cfg["parallelism"]["world_size"] = 4
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    out = subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                          "--config", str(p), "--backend", "rccl", "--shard-as", "4",
                          "--gemm-dtype", "fp8"], capture_output=True, text=True, timeout=600,
                         cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    assert not (tmp_path / f"rccl_{cfg['experiment']['name']}_shard4.json").exists()
    rec = json.load(open(tmp_path / f"rccl_{cfg['experiment']['name']}_shard4_fp8.json"))
    th = rec["throughput"]
    assert th["gemm_dtype"] == "fp8"
    assert th["hip_graph"] is True, th["hip_graph_note"]
    assert th["tokens_per_s"] > 0
    assert th["gemm_kernel_mix"]["fp8"]["calls"] > 0
    assert rec["config"]["execution"]["gemm_dtype"] == "fp8"
