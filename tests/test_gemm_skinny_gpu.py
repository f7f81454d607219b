"""Skinny-M weight-streaming GEMM (``csrc/gemm_skinny.hip``) on the GPU: exact integer products
over every path of its plan, the any-order fp32 accumulation bound on random operands, every
epilogue, padding rows / strides, determinism, graph capture, the contract fallback, the
autotuner candidate, and the decode step of the model and of ``run_tp`` running on it.

Every test that expects the kernel asserts that ``gemm.SKINNY_LAUNCHES`` moved, so a silent
fallback to another kernel cannot pass."""

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


def _gemm():
    from distributed_llm_backend_benchmark_amd.ops import gemm

    return gemm


def _skinny(x, w, bias=None, act=None, r2=None, out_dtype=torch.float32, out=None, preact=None,
            expect=1):
    """``_mfma_skinny_linear`` into a fresh (or the given) output; asserts the launch counter
    moved by ``expect``."""
    gemm = _gemm()
    if out is None:
        out = torch.empty(x.shape[0], w.shape[0], dtype=out_dtype, device=DEV)
    before = gemm.SKINNY_LAUNCHES["count"]
    gemm._mfma_skinny_linear(x, w, bias, act, r2, out, preact)
    assert gemm.SKINNY_LAUNCHES["count"] - before == expect, "skinny kernel not launched"
    return out


def _int_operands(M, N, K):
    """Integers in [-3, 4] (exact in bf16): A differs per row and per k, B is asymmetric in
    (n, k) and unrelated to A; with the exact fp64 product."""
    m = torch.arange(M, device=DEV).view(M, 1)
    n = torch.arange(N, device=DEV).view(N, 1)
    k = torch.arange(K, device=DEV).view(1, K)
    a = ((m * 7 + k * 3 + (m * k) % 5) % 8 - 3).float()
    b = ((n * 5 + k * 11 + (n // 3) + (n * k) % 7) % 8 - 3).float()
    ref = a.double() @ b.double().t()
    return a.to(BF16), b.to(BF16), ref


def _rand(*shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.rand(*shape, generator=g, device=DEV) * 2 - 1).to(BF16)


# one tile, one step / odd tile and step counts / many tiles, short K / one tile, the deepest
# K-split / 17 tiles / the real shard-8 QKV shape
INT_NK = [(16, 64), (48, 192), (4096, 512), (16, 16384), (272, 2048), (1536, 4096)]
INT_M = [1, 3, 8, 13, 16]


def test_plans_reach_every_path():
    """The integer-product shapes reach every path the plan can return: no K-split and the
    in-workgroup split, shallow and at its deepest. The kernel has no cross-workgroup split and
    no workspace: entries 2 and 3 of every plan are 1 and 0."""
    gemm = _gemm()
    ncu = gemm._num_cus(DEV)
    plans = {(N, K): gemm.skinny_plan(8, N, K, ncu) for N, K in INT_NK}
    print(plans)
    assert all(p is not None and p[0] == N // 16 for (N, K), p in plans.items())
    assert all(p[2] == 1 and p[3] == 0 for p in plans.values()), plans
    splits = {p[1] for p in plans.values()}
    assert 1 in splits and 16 in splits and any(1 < s < 16 for s in splits), plans
    assert plans[(16, 64)][1] == 1 and plans[(16, 16384)][1] == 16


@pytest.mark.parametrize("N,K", INT_NK)
def test_exact_integer_products(N, K):
    """|ref| <= 16 K < 2^24, so fp32 accumulation in any order is exact: the fp32 output equals
    the fp64 product, the bf16 output its rounding."""
    assert 16 * K < 2 ** 24
    a16, b, ref16 = _int_operands(16, N, K)
    for M in INT_M:
        a, ref = a16[:M].contiguous(), ref16[:M]
        out = _skinny(a, b)
        assert torch.equal(out.double(), ref), (M, N, K, float((out.double() - ref).abs().max()))
        outb = _skinny(a, b, out_dtype=BF16)
        assert torch.equal(outb, ref.to(BF16)), (M, N, K)


@pytest.mark.parametrize("M,N,K", [(8, 1536, 4096), (5, 48, 192)])
def test_random_operands_within_fp32_accumulation_bound(M, N, K):
    """|out - ref| <= (K + 8) 2^-24 (|x| |W|^T) for any summation order of exact bf16 products
    in fp32; the bf16 output adds its own rounding 2^-8 |ref|."""
    x, w = _rand(M, K, seed=1), _rand(N, K, seed=2)
    ref = x.double() @ w.double().t()
    bound = (K + 8) * 2.0 ** -24 * (x.double().abs() @ w.double().abs().t())
    out = _skinny(x, w)
    err = (out.double() - ref).abs()
    print(f"fp32 {M}x{N}x{K}: max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    outb = _skinny(x, w, out_dtype=BF16)
    errb = (outb.double() - ref).abs()
    boundb = bound + 2.0 ** -8 * ref.abs()
    print(f"bf16 {M}x{N}x{K}: max err/bound {float((errb / boundb).max()):.3f}")
    assert bool((errb <= boundb).all())


@pytest.mark.parametrize("out_dtype", [torch.float32, BF16])
@pytest.mark.parametrize("case", ["bias", "gelu_erf", "gelu_tanh", "residual", "all"])
def test_epilogues(case, out_dtype):
    M, N, K = 8, 320, 512
    x, w = _rand(M, K, seed=3), (_rand(N, K, seed=4).float() * 0.1).to(BF16)
    bias = _rand(N, seed=5) if case in ("bias", "all") else None
    act = {"gelu_erf": "gelu_erf", "gelu_tanh": "gelu_tanh", "all": "gelu_tanh"}.get(case)
    r2 = None
    if case in ("residual", "all"):
        r2 = _rand(M, N + 24, seed=6)[:, :N]          # row stride larger than N
        assert r2.stride(0) == N + 24
    ref = x.double() @ w.double().t()
    if bias is not None:
        ref = ref + bias.double()
    if act == "gelu_erf":
        ref = torch.nn.functional.gelu(ref)
    elif act == "gelu_tanh":
        ref = torch.nn.functional.gelu(ref, approximate="tanh")
    if r2 is not None:
        ref = ref + r2.double()
    out = _skinny(x, w, bias, act, r2, out_dtype=out_dtype)
    ratio = float((out.double() - ref).abs().max() / ref.abs().max())
    print(f"epilogue {case} {out_dtype}: max|err| / max|ref| = {ratio:.3e}")
    assert ratio < 1e-2, ratio


@pytest.mark.parametrize("M", [1, 5, 8])
def test_padding_rows_and_strides(M):
    """x is a view of a larger buffer whose other rows and columns hold NaN; out is a slice of a
    canary-filled buffer: rows >= M of x are never read, rows outside out never written."""
    N, K = 272, 2048
    buf = torch.full((16, K + 64), float("nan"), dtype=BF16, device=DEV)
    xc = _rand(M, K, seed=7)
    buf[:M, :K] = xc
    x = buf[:M, :K]
    assert x.stride(0) == K + 64
    w = _rand(N, K, seed=8)
    for dt in (torch.float32, BF16):
        ref = _skinny(xc, w, out_dtype=dt)
        obuf = torch.full((18, N), 777.0, dtype=dt, device=DEV)
        out = _skinny(x, w, out=obuf[1:M + 1])
        assert bool(torch.isfinite(out.float()).all())
        assert torch.equal(out, ref)
        assert bool((obuf[0] == 777.0).all()) and bool((obuf[M + 1:] == 777.0).all())


def test_deterministic_and_no_state_left_behind():
    for N, K in [(1536, 4096), (16, 16384)]:
        x, w = _rand(8, K, seed=9), _rand(N, K, seed=10)
        x2, w2 = _rand(5, 192, seed=11), _rand(48, 192, seed=12)
        first = _skinny(x, w)
        for _ in range(2):
            assert torch.equal(_skinny(x, w), first)
        for _ in range(3):
            _skinny(x2, w2)                          # another shape on the same stream
            assert torch.equal(_skinny(x, w), first)


def test_first_call_inside_graph_capture():
    """The first skinny call of a shape (one no other test uses) happens while capturing on the
    capture's own fresh stream; replays with x rewritten equal the eager result bit for bit."""
    M, N, K = 7, 208, 1216
    w = _rand(N, K, seed=13)
    xs = [_rand(M, K, seed=20 + i) for i in range(3)]
    x = torch.zeros(M, K, dtype=BF16, device=DEV)
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _skinny(x, w, out=out)
    for xi in xs:
        x.copy_(xi)
        g.replay()
        torch.cuda.synchronize()
        got = out.clone()
        assert torch.equal(got, _skinny(xi, w))


def test_outside_the_contract_falls_back():
    gemm = _gemm()
    from distributed_llm_backend_benchmark_amd.ops import _lib

    def check(x, w, preact=None):
        out = torch.empty(x.shape[0], w.shape[0], dtype=torch.float32, device=DEV)
        _skinny(x, w, out=out, preact=preact, expect=0)
        ref = x.float() @ w.float().t()
        torch.testing.assert_close(out, ref, rtol=2e-2, atol=2e-2 * float(ref.abs().max()))

    check(_rand(17, 128, seed=30), _rand(32, 128, seed=31))            # M = 17
    check(_rand(8, 128, seed=32), _rand(24, 128, seed=33))             # N = 24
    check(_rand(8, 96, seed=34), _rand(32, 96, seed=35))               # K = 96
    check(_rand(8, 128, seed=36), _rand(32, 128, seed=37),
          preact=torch.empty(8, 32, dtype=BF16, device=DEV))           # a pre-activation output
    xm = _rand(8, 136, seed=38)[:, 1:129]                              # rows not 16-byte aligned
    assert xm.data_ptr() % 16 != 0
    check(xm, _rand(32, 128, seed=39))
    # the C entry point itself refuses M = 17 and launches nothing
    x, w = _rand(17, 128, seed=40), _rand(32, 128, seed=41)
    out = torch.full((17, 32), 5.0, dtype=torch.float32, device=DEV)
    rc = _lib.lib().dlbb_gemm_bf16_nt_skinny(
        x.data_ptr(), 128, w.data_ptr(), 128, out.data_ptr(), 17, 32, 128, None, None, 0, 0, 1,
        gemm._num_cus(DEV), _lib.stream(DEV))
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == 5.0).all())
    assert gemm.skinny_plan(17, 32, 128, 256) is None


def test_autotuner_offers_skinny_only_at_small_m(monkeypatch):
    gemm = _gemm()
    from distributed_llm_backend_benchmark_amd.ops import linear

    monkeypatch.setenv("DLBB_GEMM", "auto")
    w = _rand(1536, 4096, seed=50)
    x8, x32 = _rand(8, 4096, seed=51), _rand(32, 4096, seed=52)
    for k in [k for k in gemm.CHOICES if k[:3] in ((8, 1536, 4096), (32, 1536, 4096))]:
        del gemm.CHOICES[k]
    linear(x8, w)
    kind, key, times, best = gemm.TUNE_LOG[-1]
    assert key[:3] == (8, 1536, 4096) and "mfma_skinny" in times, times
    print(f"tuned M=8: {times} -> {best}")
    linear(x32, w)
    kind, key, times, best = gemm.TUNE_LOG[-1]
    assert key[:3] == (32, 1536, 4096) and "mfma_skinny" not in times, times
    monkeypatch.setenv("DLBB_GEMM", "mfma_skinny")
    before = gemm.SKINNY_LAUNCHES["count"]
    y = linear(x8, w)
    assert gemm.SKINNY_LAUNCHES["count"] == before + 1
    ref = x8.float() @ w.float().t()
    torch.testing.assert_close(y.float(), ref, rtol=2e-2, atol=2e-2 * float(ref.abs().max()))


def test_model_decode_steps_run_on_the_skinny_kernel(monkeypatch):
    """Batch 8: 48 prompt tokens + 16 decode steps under DLBB_GEMM=mfma_skinny against the full
    64-token forward under the default dispatch (3e-2 of max|ref|, the TP-vs-dense bound); the
    four linears of both layers run on the kernel in every decode step, the prefill (M = 384)
    on none."""
    gemm = _gemm()
    from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
    from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

    model = LLM(comm=Comm(0, 1, 0, "gloo", DEV), num_heads=4, hidden_size=256, num_layers=2,
                ffn_intermediate=1024, seed=11, init_std=0.05, attention="flash")
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(8, 64, 256, generator=g, device=DEV).to(BF16)
    monkeypatch.delenv("DLBB_GEMM", raising=False)
    ref = model(x).float()
    monkeypatch.setenv("DLBB_GEMM", "mfma_skinny")
    before = gemm.SKINNY_LAUNCHES["count"]
    cache = model.new_kv_cache(8, 64)
    rows = [model(x[:, :48].contiguous(), kv_cache=cache)]
    for t in range(48, 64):
        rows.append(model(x[:, t:t + 1].contiguous(), kv_cache=cache))
    got = torch.cat(rows, dim=1).float()
    torch.cuda.synchronize()
    assert gemm.SKINNY_LAUNCHES["count"] - before == 16 * 2 * 4
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"decode on mfma_skinny vs full forward: {err:.3e}")
    assert err < 3e-2, err


def _cfg(tmp_path):
    import yaml

    cfg = yaml.safe_load(open(os.path.join(REPO, "config", "baseline_config.yaml")))
    cfg["model"].update(hidden_size=512, num_layers=2, num_heads=8, ffn_intermediate=2048,
                        init_std=0.02)
    cfg["input"].update(batch_size=2, sequence_length=64)
    cfg["execution"].update(warmup_iterations=1, benchmark_iterations=3)
    cfg["parallelism"]["world_size"] = 1
    cfg["experiment"]["output_dir"] = str(tmp_path)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return p, cfg["experiment"]["name"]


@pytest.mark.parametrize("forced", [True, False])
def test_run_tp_decode(tmp_path, forced):
    """``run_tp --decode`` at M = 2: forced onto the kernel it still replays a HIP graph; left
    to the autotuner every decode shape has an ``mfma_skinny`` timing."""
    p, name = _cfg(tmp_path)
    env = dict(os.environ)
    env.pop("DLBB_GEMM", None)
    if forced:
        env["DLBB_GEMM"] = "mfma_skinny"
    out = subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                          "--config", str(p), "--backend", "rccl", "--decode", "8",
                          "--attention", "flash"], capture_output=True, text=True, timeout=600,
                         cwd=REPO, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.load(open(tmp_path / f"rccl_{name}_decode8.json"))["decode"]
    assert d["timing_mode"] == "hip_graph_replay", d["hip_graph_note"]
    if not forced:
        tuned = d["gemm_kernel_mix"]["tuned"]
        assert tuned and all("mfma_skinny" in t["ms"] for t in tuned), tuned
        print(d["gemm_kernel_mix"]["shapes_by_choice"])
