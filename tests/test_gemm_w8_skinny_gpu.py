"""Weight-only FP8 (W8A16) skinny GEMM (``csrc/gemm_skinny.hip``) on the GPU: exact integer
products over every path of its plan, every e4m3 code dequantised exactly, the any-order fp32
accumulation bound on random operands, every epilogue, padding rows / strides, determinism,
graph capture, the contract refusals, and the decode step of the model and of ``run_tp`` on it.

Every test that expects the kernel asserts that ``fp8.W8_LAUNCHES`` moved by the expected amount:
the op has no other GPU path, and a refused call must not move it."""

import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
BF16 = torch.bfloat16
E4M3 = torch.float8_e4m3fn


def _fp8():
    from distributed_llm_backend_benchmark_amd.ops import fp8

    return fp8


def _w8(x, wq, ws, bias=None, act=None, residual=None, out_dtype=torch.float32, out=None,
        expect=1):
    """``linear_w8``; asserts the launch counter moved by ``expect``."""
    fp8 = _fp8()
    before = fp8.W8_LAUNCHES["count"]
    y = fp8.linear_w8(x, wq, ws, bias, act, residual, out_dtype, out)
    assert fp8.W8_LAUNCHES["count"] - before == expect, "W8 skinny kernel not launched"
    return y


def _refused(*args, **kw):
    fp8 = _fp8()
    before = fp8.W8_LAUNCHES["count"]
    with pytest.raises(ValueError):
        fp8.linear_w8(*args, **kw)
    assert fp8.W8_LAUNCHES["count"] == before


def _int_operands(M, N, K):
    """Integers in [-3, 4]: x bf16, differing per row and per k; Wq e4m3fn (exact), asymmetric in
    (n, k) and unrelated to x; row scales 2^-(n % 5); with the exact fp64 result."""
    m = torch.arange(M, device=DEV).view(M, 1)
    n = torch.arange(N, device=DEV).view(N, 1)
    k = torch.arange(K, device=DEV).view(1, K)
    a = ((m * 7 + k * 3 + (m * k) % 5) % 8 - 3).float()
    b = ((n * 5 + k * 11 + (n // 3) + (n * k) % 7) % 8 - 3).float()
    bq = b.to(E4M3)
    assert torch.equal(bq.float(), b)
    ws = torch.pow(2.0, -(torch.arange(N, device=DEV) % 5).float())
    ref = (a.double() @ b.double().t()) * ws.double()
    return a.to(BF16), bq, ws, ref


def _rand(*shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.rand(*shape, generator=g, device=DEV) * 2 - 1).to(BF16)


def _quant(w):
    wq, ws = _fp8().quantize_rows(w, kernels="torch")
    return wq.contiguous(), ws.contiguous()


# one tile, one unit / odd tile and unit counts / many tiles, short K / one tile, the deepest
# K-split / 17 tiles / the real shard-8 QKV shape
INT_NK = [(16, 64), (48, 192), (4096, 512), (16, 16384), (272, 2048), (1536, 4096)]
INT_M = [1, 3, 8, 13, 16]


def test_plans_reach_every_path():
    """The integer-product shapes reach every path the plan can return: no K-split, a middle
    split and the deepest one. No cross-workgroup split and no workspace: entries 2 and 3 of
    every plan are 1 and 0."""
    from distributed_llm_backend_benchmark_amd.ops import gemm

    fp8 = _fp8()
    ncu = gemm._num_cus(DEV)
    plans = {(N, K): fp8.w8_skinny_plan(8, N, K, ncu) for N, K in INT_NK}
    print(plans)
    assert all(p is not None and p[0] == N // 16 for (N, K), p in plans.items())
    assert all(p[2] == 1 and p[3] == 0 for p in plans.values()), plans
    splits = {p[1] for p in plans.values()}
    assert 1 in splits and 16 in splits and any(1 < s < 16 for s in splits), plans
    assert plans[(16, 64)][1] == 1 and plans[(16, 16384)][1] == 16
    assert fp8.w8_skinny_plan(17, 32, 128, ncu) is None


@pytest.mark.parametrize("N,K", INT_NK)
def test_exact_integer_products(N, K):
    """|acc| <= 16 K < 2^24 and the scale is a power of two, so fp32 accumulation in any order
    and the scaling are exact: the fp32 output equals the fp64 result, the bf16 output its
    rounding."""
    assert 16 * K < 2 ** 24
    a16, bq, ws, ref16 = _int_operands(16, N, K)
    for M in INT_M:
        a, ref = a16[:M].contiguous(), ref16[:M]
        out = _w8(a, bq, ws)
        assert torch.equal(out.double(), ref), (M, N, K, float((out.double() - ref).abs().max()))
        outb = _w8(a, bq, ws, out_dtype=BF16)
        assert torch.equal(outb, ref.to(BF16)), (M, N, K)


def test_every_e4m3_code_dequantises_exactly():
    """Row n of Wq holds byte n (the two NaN codes replaced by 0) at column n % 64 and zero
    elsewhere; against x = 1 and unit scales the output is the value of each code: subnormals,
    +-0 and +-448 included."""
    codes = torch.arange(256, device=DEV, dtype=torch.int32)
    codes[0x7f] = 0
    codes[0xff] = 0
    raw = torch.zeros(256, 64, dtype=torch.uint8, device=DEV)
    raw[torch.arange(256, device=DEV), torch.arange(256, device=DEV) % 64] = codes.to(torch.uint8)
    wq = raw.view(E4M3)
    x = torch.ones(1, 64, dtype=BF16, device=DEV)
    ws = torch.ones(256, dtype=torch.float32, device=DEV)
    out = _w8(x, wq, ws)
    want = wq.float().sum(1).view(1, 256)
    assert float(want.max()) == 448.0 and float(want.min()) == -448.0
    assert float(want[want > 0].min()) == 2.0 ** -9           # the smallest subnormal
    assert torch.equal(out, want), (out - want).abs().max()


@pytest.mark.parametrize("M,N,K", [(8, 1536, 4096), (5, 48, 192)])
def test_random_operands_within_fp32_accumulation_bound(M, N, K):
    """|out - ref| <= ((K + 8) 2^-24 (|x| |wq|^T) + 2^-24 |x wq^T|) ws: any summation order of
    exact products in fp32 plus one rounding for the scale; the bf16 output adds 2^-8 |ref|."""
    x, w = _rand(M, K, seed=1), _rand(N, K, seed=2)
    wq, ws = _quant(w)
    xd, wd, sd = x.double(), wq.float().double(), ws.double()
    dot = xd @ wd.t()
    ref = dot * sd
    bound = ((K + 8) * 2.0 ** -24 * (xd.abs() @ wd.abs().t()) + 2.0 ** -24 * dot.abs()) * sd
    out = _w8(x, wq, ws)
    err = (out.double() - ref).abs()
    print(f"fp32 {M}x{N}x{K}: max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    outb = _w8(x, wq, ws, out_dtype=BF16)
    errb = (outb.double() - ref).abs()
    boundb = bound + 2.0 ** -8 * ref.abs()
    print(f"bf16 {M}x{N}x{K}: max err/bound {float((errb / boundb).max()):.3f}")
    assert bool((errb <= boundb).all())


@pytest.mark.parametrize("out_dtype", [torch.float32, BF16])
@pytest.mark.parametrize("case", ["bias", "gelu_erf", "gelu_tanh", "residual", "all"])
def test_epilogues(case, out_dtype):
    M, N, K = 8, 320, 512
    x = _rand(M, K, seed=3)
    wq, ws = _quant((_rand(N, K, seed=4).float() * 0.1).to(BF16))
    bias = _rand(N, seed=5) if case in ("bias", "all") else None
    act = {"gelu_erf": "gelu_erf", "gelu_tanh": "gelu_tanh", "all": "gelu_tanh"}.get(case)
    r2 = None
    if case in ("residual", "all"):
        r2 = _rand(M, N + 24, seed=6)[:, :N]          # row stride larger than N
        assert r2.stride(0) == N + 24
    ref = (x.double() @ wq.float().double().t()) * ws.double()
    if bias is not None:
        ref = ref + bias.double()
    if act == "gelu_erf":
        ref = torch.nn.functional.gelu(ref)
    elif act == "gelu_tanh":
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
    if r2 is not None:
        ref = ref + r2.double()
    out = _w8(x, wq, ws, bias, act, r2, out_dtype=out_dtype)
    ratio = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"epilogue {case} {out_dtype}: max|err| / max|ref| = {ratio:.3e}")
    assert ratio < 1e-2, ratio


@pytest.mark.parametrize("M", [1, 5, 8])
def test_padding_rows_and_strides(M):
    """x is a view of a NaN-filled buffer, Wq a view (row stride K + 16) of a buffer whose other
    bytes are the e4m3 NaN code, out a slice of a canary-filled buffer: rows >= M of x and bytes
    outside the operands are never read, rows outside out never written."""
    N, K = 272, 2048
    buf = torch.full((16, K + 64), float("nan"), dtype=BF16, device=DEV)
    xc = _rand(M, K, seed=7)
    buf[:M, :K] = xc
    x = buf[:M, :K]
    assert x.stride(0) == K + 64
    wqc, ws = _quant(_rand(N, K, seed=8))
    wbuf = torch.full((N, K + 16), 0x7f, dtype=torch.uint8, device=DEV)
    wbuf[:, :K] = wqc.view(torch.uint8)
    wq = wbuf.view(E4M3)[:, :K]
    assert wq.stride(0) == K + 16 and wq.data_ptr() % 16 == 0
    for dt in (torch.float32, BF16):
        ref = _w8(xc, wqc, ws, out_dtype=dt)
        obuf = torch.full((18, N), 777.0, dtype=dt, device=DEV)
        out = _w8(x, wq, ws, out=obuf[1:M + 1])
        assert bool(torch.isfinite(out.float()).all())
        assert torch.equal(out, ref)
        assert bool((obuf[0] == 777.0).all()) and bool((obuf[M + 1:] == 777.0).all())


def test_deterministic_and_no_state_left_behind():
    x2 = _rand(5, 192, seed=11)
    wq2, ws2 = _quant(_rand(48, 192, seed=12))
    for N, K in [(1536, 4096), (16, 16384)]:
        x = _rand(8, K, seed=9)
        wq, ws = _quant(_rand(N, K, seed=10))
        first = _w8(x, wq, ws)
        for _ in range(2):
            assert torch.equal(_w8(x, wq, ws), first)
        for _ in range(3):
            _w8(x2, wq2, ws2)                        # another shape on the same stream
            assert torch.equal(_w8(x, wq, ws), first)


def test_first_call_inside_graph_capture():
    """The first call of a shape (one no other test uses) happens while capturing on the
    capture's own fresh stream; replays with x rewritten equal the eager result bit for bit."""
    M, N, K = 7, 208, 1216
    wq, ws = _quant(_rand(N, K, seed=13))
    xs = [_rand(M, K, seed=20 + i) for i in range(3)]
    x = torch.zeros(M, K, dtype=BF16, device=DEV)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _w8(x, wq, ws, out=out)
    for xi in xs:
        x.copy_(xi)
        g.replay()
        torch.cuda.synchronize()
        got = out.clone()
        assert torch.equal(got, _w8(xi, wq, ws))


def test_contract_violations_raise_and_launch_nothing():
    from distributed_llm_backend_benchmark_amd.ops import _lib, gemm

    def ops(M, N, K, seed):
        wq, ws = _quant(_rand(N, K, seed=seed + 1))
        return _rand(M, K, seed=seed), wq, ws

    _refused(*ops(17, 32, 128, 30))                                    # M = 17
    _refused(*ops(8, 24, 128, 32))                                     # N = 24
    _refused(*ops(8, 32, 96, 34))                                      # K = 96
    x, wq, ws = ops(8, 32, 128, 36)
    xm = _rand(8, 136, seed=38)[:, 1:129]                              # rows not 16-byte aligned
    assert xm.data_ptr() % 16 != 0
    _refused(xm, wq, ws)
    wbuf = torch.zeros(32, 128 + 8, dtype=torch.uint8, device=DEV).view(E4M3)
    wv = wbuf[:, :128]                                                 # row stride K + 8
    assert wv.stride(0) == 136 and wv.data_ptr() % 16 == 0
    _refused(x, wv, ws)
    _refused(x, _rand(32, 128, seed=39), ws)                           # a bf16 wq
    _refused(x.to(torch.float16), wq, ws)                              # an fp16 x
    _w8(x, wq, ws)                                                     # the operands themselves run
    # the C entry point itself refuses M = 17 and launches nothing
    x17, wq, ws = ops(17, 32, 128, 40)
    out = torch.full((17, 32), 5.0, dtype=torch.float32, device=DEV)
    rc = _lib.lib().dlbb_gemm_w8_nt_skinny(
        x17.data_ptr(), 128, wq.data_ptr(), 128, ws.data_ptr(), out.data_ptr(), 17, 32, 128,
        None, None, 0, 0, 1, gemm._num_cus(DEV), _lib.stream(DEV))
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == 5.0).all())


def _decode(model, x, prompt):
    cache = model.new_kv_cache(x.shape[0], x.shape[1])
    rows = [model(x[:, :prompt].contiguous(), kv_cache=cache)]
    torch.cuda.synchronize()
    marks = (_fp8().W8_LAUNCHES["count"], _gemm().SKINNY_LAUNCHES["count"])
    for t in range(prompt, x.shape[1]):
        rows.append(model(x[:, t:t + 1].contiguous(), kv_cache=cache))
    torch.cuda.synchronize()
    return torch.cat(rows[1:], dim=1).float(), marks


def _gemm():
    from distributed_llm_backend_benchmark_amd.ops import gemm

    return gemm


def test_model_decode_steps_stream_fp8_weights(monkeypatch):
    """Batch 8: 48 prompt tokens, then 16 decode steps with ``decode_weight_dtype="fp8"``. The
    four linears of both layers run on the W8 kernel in every decode step and in no prefill; the
    bf16 skinny kernel (forced for every bf16 linear of M <= 16) runs in none of them. The decode
    outputs match the same model in torch (same weights, ``kernels="torch"``, sdpa, same knob)
    within 3e-2 of max|ref|, the TP-vs-dense bound; the distance to the all-bf16 decode is printed
    and held below the fp8 ``--check-dense`` tolerance, 0.25."""
    fp8, gemm = _fp8(), _gemm()
    from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
    from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

    monkeypatch.setenv("DLBB_GEMM", "mfma_skinny")

    def make(**kw):
        return LLM(comm=Comm(0, 1, 0, "gloo", DEV), num_heads=4, hidden_size=256, num_layers=2,
                   ffn_intermediate=1024, seed=11, init_std=0.05, **kw)

    model = make(attention="flash", decode_weight_dtype="fp8")
    ref_model = make(attention="sdpa", kernels="torch", decode_weight_dtype="fp8")
    ref_model.load_state_dict(model.state_dict())
    bf16_model = make(attention="flash")
    bf16_model.load_state_dict(model.state_dict())
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(8, 64, 256, generator=g, device=DEV).to(BF16)

    w8_0, sk_0 = fp8.W8_LAUNCHES["count"], gemm.SKINNY_LAUNCHES["count"]
    got, (w8_1, sk_1) = _decode(model, x, 48)
    assert w8_1 - w8_0 == 0, "the prefill ran on the W8 kernel"
    assert fp8.W8_LAUNCHES["count"] - w8_1 == 16 * 2 * 4
    assert gemm.SKINNY_LAUNCHES["count"] - sk_1 == 0
    ref, _ = _decode(ref_model, x, 48)
    assert fp8.W8_LAUNCHES["count"] - w8_1 == 16 * 2 * 4, "the torch reference launched the kernel"
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"W8 decode, HIP vs torch: {err:.3e}")
    assert err < 3e-2, err
    sk_2 = gemm.SKINNY_LAUNCHES["count"]
    plain, _ = _decode(bf16_model, x, 48)
    assert gemm.SKINNY_LAUNCHES["count"] - sk_2 == 16 * 2 * 4
    dist = float((got - plain).abs().max() / plain.abs().max())
    print(f"W8 decode vs all-bf16 decode: {dist:.3e}")
    assert dist < 0.25, dist
    with pytest.raises(ValueError):
        make(attention="flash", decode_weight_dtype="fp8").new_kv_cache(17, 64)


def _cfg(tmp_path, **model):
    import yaml

    cfg = yaml.safe_load(open(os.path.join(REPO, "config", "baseline_config.yaml")))
    cfg["model"].update(hidden_size=512, num_layers=2, num_heads=8, ffn_intermediate=2048,
                        init_std=0.02)
    cfg["model"].update(model)
    cfg["input"].update(batch_size=2, sequence_length=64)
    cfg["execution"].update(warmup_iterations=1, benchmark_iterations=3)
    cfg["parallelism"]["world_size"] = 1
    cfg["experiment"]["output_dir"] = str(tmp_path)
    return cfg


def _run_tp(tmp_path, cfg, *extra):
    import yaml

    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, DLBB_GEMM="mfma_skinny")
    return subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                           "--config", str(p), "--backend", "rccl", "--attention", "flash",
                           "--decode-weights", "fp8", *extra], capture_output=True, text=True,
                          timeout=600, cwd=REPO, env=env)


def test_run_tp_decode_weights_fp8(tmp_path):
    cfg = _cfg(tmp_path)
    out = _run_tp(tmp_path, cfg, "--decode", "8")
    assert out.returncode == 0, out.stderr[-3000:]
    name = cfg["experiment"]["name"]
    d = json.load(open(tmp_path / f"rccl_{name}_decode8_w8.json"))["decode"]
    assert d["timing_mode"] == "hip_graph_replay", d["hip_graph_note"]
    assert d["weight_dtype"] == "fp8" and d["w8_launches_per_step"] == 8
    # per layer: QKV 1536 x 512, out 512 x 512, up 2048 x 512, down 512 x 2048 e4m3 bytes, one
    # fp32 scale per output row, two LayerNorms of 2 x 512 bf16; plus the final LayerNorm
    linears = 1536 * 512 + 512 * 512 + 2048 * 512 + 512 * 2048
    scales = 4 * (1536 + 512 + 2048 + 512)
    want = 2 * (linears + scales + 2 * 2 * 512 * 2) + 2 * 512 * 2
    assert d["weight_stream_bytes_per_rank"] == want == 6338560
    assert d["weight_bytes_per_rank"] > want


@pytest.mark.parametrize("case", ["no_decode", "batch17", "hidden480"])
def test_run_tp_decode_weights_fp8_refusals(tmp_path, case):
    cfg, extra = _cfg(tmp_path), ["--decode", "8"]
    if case == "no_decode":
        extra = []
    elif case == "batch17":
        cfg["input"]["batch_size"] = 17
    else:                   # every divisibility term holds except hidden_size % 64
        cfg = _cfg(tmp_path, hidden_size=480)
    out = _run_tp(tmp_path, cfg, *extra)
    assert out.returncode == 1, out.stderr[-3000:]
    assert "ERROR" in out.stdout
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".json")]
