"""Weight-only MXFP4 (W4A16) decode, CPU side (torch path; gloo world 1): the quantiser bit for
bit against a slow reference written here, its error, the op's formula and epilogues, the shape
contract's edges, the weight cache, config validation, the model's decode steps taking the W4
path (and its prefill not), and the ``run_tp --decode-weights mxfp4`` record."""

import copy
import json
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
from distributed_llm_backend_benchmark_amd.ops import mxfp4
from distributed_llm_backend_benchmark_amd.parallel.comm import Comm
from distributed_llm_backend_benchmark_amd.utils.config import (DEFAULT_CONFIG, ConfigError,
                                                                check_w4_shapes, validate_config)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _rand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * 2 - 1).to(BF16)


def _randn(*shape, seed, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(BF16)


def _ref_quantize(w):
    """The issue's rule, one element at a time in Python floats (doubles: every step is exact)."""
    N, K = w.shape
    rows = w.float().tolist()
    codes = [[0] * (K // 2) for _ in range(N)]
    scales = [[0] * (K // 32) for _ in range(N)]
    for n in range(N):
        for blk in range(K // 32):
            xs = rows[n][32 * blk:32 * blk + 32]
            amax = max(abs(v) for v in xs)
            if amax == 0:
                b = 127
            else:
                b = min(max(math.frexp(amax)[1] - 1 - 2 + 127, 2), 254)
            scales[n][blk] = b
            for i, xv in enumerate(xs):
                a = min(abs(xv) / 2.0 ** (b - 127), 6.0)
                best = min(range(8), key=lambda c: (abs(GRID[c] - a), c % 2))   # ties: even code
                code = best | (8 if xv < 0 else 0)
                k = 32 * blk + i
                codes[n][k // 2] |= code << (4 * (k % 2))
    return (torch.tensor(codes, dtype=torch.uint8), torch.tensor(scales, dtype=torch.uint8))


def _quantiser_inputs():
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5,
                         -3.5, -5.0, 6.0, -6.0, 0.0, -0.0, 4.0, 3.0, 2.0, 1.5, 1.0, 0.5, -4.0,
                         -3.0, -2.0, -1.5, -1.0, -0.5, 4.5, 5.5])
    zero = torch.zeros(32)
    pow2 = _randn(32, seed=20).float().clamp(-3, 3)
    pow2[7] = -4.0                                                    # amax = 2^2 exactly
    below = _randn(32, seed=21).float().clamp(-3, 3)
    below[11] = 7.96875                                               # bf16 just below 8: -> 6
    big = _randn(32, seed=22).float() * 1e37
    big[3] = torch.finfo(BF16).max
    tiny = torch.zeros(32)
    tiny[5] = 2.0 ** -133                                             # smallest bf16 subnormal
    tiny[9] = -(2.0 ** -130)
    small = _randn(32, seed=23).float() * 2.0 ** -126                 # b clamps to 2 here too
    special = torch.stack([torch.cat([ties, zero, pow2, below]),
                           torch.cat([big, tiny, small, ties * 2.0 ** -40])]).to(BF16)
    rows = [_randn(4, 128, seed=30 + i, std=std) for i, std in enumerate((1.0, 0.02, 1e-30))]
    return torch.cat(rows + [special])


def test_quantiser_is_bit_equal_to_the_slow_reference():
    w = _quantiser_inputs()
    assert float(w[:4].float().abs().max()) > 1 and float(w[8:12].float().abs().max()) < 1e-29
    codes, scales = ops.quantize_mxfp4(w)
    rc, rs = _ref_quantize(w)
    assert codes.dtype == torch.uint8 and codes.shape == (14, 64)
    assert scales.dtype == torch.uint8 and scales.shape == (14, 4)
    assert torch.equal(scales, rs)
    assert torch.equal(codes, rc)
    assert int(scales.min()) >= 2 and int(scales.max()) <= 252
    # the named cases
    sp = scales[12:]
    assert sp[0].tolist() == [127, 127, 127, 127]          # ties, zero block, 4, 7.97 -> 2^0
    assert sp[1, 0] == 252 and sp[1, 1] == 2 and sp[1, 2] == 2
    d = ops.dequantize_mxfp4(codes, scales)
    assert d.dtype == torch.float32 and d.shape == w.shape
    assert torch.equal(d.to(BF16).float(), d)              # every value is a bf16
    assert torch.isfinite(d).all()
    nz = d[d != 0].abs()
    assert float(nz.min()) >= 2.0 ** -126                   # and a normal one
    assert d[12, :8].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, -0.0]
    assert d[12, 96 + 11] == 6.0 and d[12, 64 + 7] == -4.0
    assert d[13, 3] == 6 * 2.0 ** 125 and d[13, 32 + 5] == 0
    # a second call with the rows chunked one by one gives the same bits
    old, mxfp4._CHUNK_ELEMS = mxfp4._CHUNK_ELEMS, 128
    try:
        c2, s2 = ops.quantize_mxfp4(w)
    finally:
        mxfp4._CHUNK_ELEMS = old
    assert torch.equal(c2, codes) and torch.equal(s2, scales)


@pytest.mark.parametrize("std", [1.0, 0.02])
def test_quantisation_error(std):
    """The rule's own relative Frobenius error is 0.114-0.115 at both magnitudes, for the weight
    and for a product; [0.09, 0.14] is that +- 20 %: a wrong exponent or a missing saturation
    falls outside."""
    w = _randn(512, 1024, seed=40, std=std)
    d = ops.dequantize_mxfp4(*ops.quantize_mxfp4(w))
    rel = float((d - w.float()).norm() / w.float().norm())
    x = _randn(16, 1024, seed=41)
    y, yd = x.float() @ w.float().t(), x.float() @ d.t()
    relp = float((yd - y).norm() / y.norm())
    print(f"std {std}: weight rel err {rel:.4f}, product rel err {relp:.4f}")
    assert 0.09 <= rel <= 0.14, rel
    assert 0.09 <= relp <= 0.14, relp


@pytest.mark.parametrize("out_dtype", [torch.float32, BF16])
@pytest.mark.parametrize("case", ["plain", "bias", "gelu_erf", "gelu_tanh", "residual", "all"])
def test_linear_w4_torch_formula(case, out_dtype):
    M, N, K = 5, 48, 192
    x = _rand(2, M, K, seed=1)                                        # leading dims are kept
    codes, scales = ops.quantize_mxfp4(_rand(N, K, seed=2))
    bias = _rand(N, seed=3) if case in ("bias", "all") else None
    act = {"gelu_erf": "gelu_erf", "gelu_tanh": "gelu_tanh", "all": "gelu_tanh"}.get(case)
    res = _rand(2, M, N, seed=4) if case in ("residual", "all") else None
    ref = x.float() @ ops.dequantize_mxfp4(codes, scales).t()
    if bias is not None:
        ref = ref + bias.float()
    if act == "gelu_erf":
        ref = F.gelu(ref)
    elif act == "gelu_tanh":
        ref = F.gelu(ref, approximate="tanh")
    if res is not None:
        ref = ref + res.float()
    before = mxfp4.W4_LAUNCHES["count"]
    out = ops.linear_w4(x, codes, scales, bias, act, res, out_dtype)
    assert mxfp4.W4_LAUNCHES["count"] == before                       # no kernel on the CPU
    assert out.shape == (2, M, N) and out.dtype == out_dtype
    assert torch.equal(out, ref.to(out_dtype))                        # the same formula
    into = torch.empty(2, M, N, dtype=out_dtype)
    assert ops.linear_w4(x, codes, scales, bias, act, res, out_dtype, out=into) is into
    assert torch.equal(into, out)
    with pytest.raises(ValueError):
        ops.linear_w4(x, codes, scales[:, :-1], out_dtype=out_dtype)
    with pytest.raises(ValueError):
        ops.linear_w4(x, codes[:, :-16], scales, out_dtype=out_dtype)


@pytest.mark.parametrize("M,ok", [(0, False), (1, True), (16, True), (17, False)])
def test_w4_contract_m_edges(M, ok):
    assert (ops.w4_contract_error(M, 32, 128) is None) is ok


@pytest.mark.parametrize("N,K,ok", [(16, 128, True), (24, 128, False), (16, 192, False),
                                    (16, 64, False), (16, 256, True)])
def test_w4_contract_shape_edges(N, K, ok):
    why = ops.w4_contract_error(8, N, K)
    assert (why is None) is ok
    if not ok:
        assert str(N if N % 16 else K) in why


def test_w4_linear_has_a_weight_cache_of_its_own():
    from distributed_llm_backend_benchmark_amd.ops import fp8

    mxfp4.clear_weight_cache()
    fp8.clear_weight_cache()
    w = torch.nn.Parameter(_rand(32, 128, seed=5), requires_grad=False)
    x = _rand(4, 128, seed=6)
    y = ops.w4_linear(x, w)
    codes, scales = ops.quantize_weight_mxfp4(w)
    y2 = ops.w4_linear(x, w)
    c2, s2 = ops.quantize_weight_mxfp4(w)
    assert c2 is codes and s2 is scales                               # quantised once
    assert torch.equal(y, y2) and torch.equal(y, ops.linear_w4(x, codes, scales))
    assert w.data_ptr() not in fp8._WCACHE                            # e4m3 entries live there
    assert torch.equal(codes, ops.quantize_mxfp4(w)[0])
    w.mul_(2)                                                         # an in-place update
    c3, s3 = ops.quantize_weight_mxfp4(w)
    assert c3 is not codes and torch.equal(c3, codes) and torch.equal(s3, scales + 1)
    with pytest.raises(ValueError):
        ops.w4_linear(_rand(4, 256, seed=8), w)
    key = w.data_ptr()
    del w
    assert key not in mxfp4._W4CACHE                                  # dropped with the weight


def test_config_validation():
    cfg = validate_config(copy.deepcopy(DEFAULT_CONFIG))
    assert cfg["execution"]["decode_weight_dtype"] == "bf16"

    def cfg_with(world=1, **model):
        c = copy.deepcopy(DEFAULT_CONFIG)
        c["execution"]["decode_weight_dtype"] = "mxfp4"
        c["parallelism"]["world_size"] = world
        c["model"].update(model)
        return c

    assert validate_config(cfg_with())["execution"]["decode_weight_dtype"] == "mxfp4"
    validate_config(cfg_with(world=8))
    with pytest.raises(ConfigError, match="hidden_size to be a multiple of 128"):
        validate_config(cfg_with(hidden_size=192))
    with pytest.raises(ConfigError, match=r"hidden_size / 4 ranks"):      # 256 / 4 = 64 per rank
        validate_config(cfg_with(world=4, hidden_size=256))
    with pytest.raises(ConfigError, match=r"ffn_intermediate / 8 ranks"):
        validate_config(cfg_with(world=8, ffn_intermediate=4096 + 512))
    with pytest.raises(ConfigError, match=r"hidden_size / 3 ranks"):
        check_w4_shapes(cfg_with(), 3)
    check_w4_shapes(cfg_with(), 8)
    bad = copy.deepcopy(DEFAULT_CONFIG)
    bad["execution"]["gemm_dtype"] = "mxfp4"                          # the GEMM knob keeps refusing
    with pytest.raises(ConfigError, match="gemm_dtype"):
        validate_config(bad)


def _model(**kw):
    comm = Comm(0, 1, 0, "gloo", torch.device("cpu"))
    return LLM(hidden_size=256, num_layers=2, num_heads=4, ffn_intermediate=1024, comm=comm,
               seed=3, init_std=0.05, kernels="torch", attention="sdpa", **kw)


def test_model_decode_steps_take_the_w4_path(monkeypatch):
    calls = []
    real = ops.w4_linear

    def counted(x, w, *a, **kw):
        calls.append((x.numel() // x.shape[-1], tuple(w.shape)))
        return real(x, w, *a, **kw)

    monkeypatch.setattr(ops, "w4_linear", counted)
    model = _model(decode_weight_dtype="mxfp4")
    x = torch.randn(2, 16, 256, generator=torch.Generator().manual_seed(1)).to(BF16)
    model(x)                                                          # no cache: bf16 weights
    cache = model.new_kv_cache(2, 16)
    model(x[:, :8].contiguous(), kv_cache=cache)                      # the prefill
    assert calls == []
    rows = [model(x[:, t:t + 1].contiguous(), kv_cache=cache) for t in range(8, 16)]
    assert len(calls) == 8 * 2 * 4 and all(m == 2 for m, _ in calls)
    assert {s for _, s in calls} == {(768, 256), (256, 256), (1024, 256), (256, 1024)}
    # the same steps by a bf16 model whose linears hold the dequantised weights (each one a
    # bf16, so the copy is exact); its prefill cache comes from the true weights, as above
    deq = _model()
    deq.load_state_dict(model.state_dict())
    cache = deq.new_kv_cache(2, 16)
    deq(x[:, :8].contiguous(), kv_cache=cache)
    for name, p in deq.named_parameters():
        if p.dim() == 2:
            p.copy_(ops.dequantize_mxfp4(*ops.quantize_mxfp4(p)).to(BF16))
    ref = torch.cat([deq(x[:, t:t + 1].contiguous(), kv_cache=cache) for t in range(8, 16)], 1)
    assert len(calls) == 64
    got = torch.cat(rows, 1).float()
    rel = float((got - ref.float()).abs().max() / ref.float().abs().max())
    print(f"decode vs the dequantised-weight forward: {rel:.3e} of max|ref|")
    assert rel < 3e-2, rel


def test_model_decode_weight_bytes_and_knob_checks():
    model = _model(decode_weight_dtype="mxfp4")
    linears = 768 * 256 + 256 * 256 + 1024 * 256 + 256 * 1024
    ln = 2 * 256 * 2                                                  # weight + bias, bf16
    assert model.decode_weight_bytes() == 2 * (linears // 2 + linears // 32 + 2 * ln) + ln
    assert model.get_memory_footprint() == 2 * (2 * linears + 2 * ln) + ln
    with pytest.raises(ValueError, match="gemm_dtype"):
        _model(decode_weight_dtype="mxfp4", gemm_dtype="fp8")
    with pytest.raises(ValueError):
        _model(gemm_dtype="mxfp4")
    model.new_kv_cache(17, 4)              # the torch path has no 16-row limit


def _run_tp(cfg_path, *extra):
    return subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                           "--config", str(cfg_path), "--backend", "gloo", "--device", "cpu",
                           *extra], capture_output=True, text=True, timeout=600, cwd=REPO)


def test_run_tp_decode_weights_record_on_cpu(tmp_path):
    import yaml

    cfg = yaml.safe_load(open(os.path.join(REPO, "config", "baseline_config.yaml")))
    cfg["model"].update(hidden_size=128, num_layers=2, num_heads=2, ffn_intermediate=256,
                        init_std=0.05)
    cfg["input"].update(batch_size=2, sequence_length=16)
    cfg["execution"].update(warmup_iterations=1, benchmark_iterations=2, attention="sdpa",
                            kernels="torch")
    cfg["parallelism"]["world_size"] = 1
    cfg["experiment"]["output_dir"] = str(tmp_path)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    name = cfg["experiment"]["name"]

    out = _run_tp(p, "--decode-weights", "mxfp4")
    assert out.returncode == 1 and "ERROR" in out.stdout, out.stderr[-3000:]
    assert "needs decode tokens" in out.stdout
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".json")]

    out = _run_tp(p, "--decode", "4", "--decode-weights", "mxfp4")
    assert out.returncode == 0, out.stderr[-3000:]
    assert not (tmp_path / f"gloo_{name}_decode4.json").exists()
    rec = json.load(open(tmp_path / f"gloo_{name}_decode4_w4.json"))
    d = rec["decode"]
    assert rec["config"]["execution"]["decode_weight_dtype"] == "mxfp4"
    assert d["weight_dtype"] == "mxfp4"
    assert d["w4_launches_per_step"] == 0                             # torch path: no kernel
    assert "w8_launches_per_step" not in d
    linears = 384 * 128 + 128 * 128 + 256 * 128 + 128 * 256
    ln = 2 * 128 * 2
    want = 2 * (linears // 2 + linears // 32 + 2 * ln) + ln
    assert d["weight_stream_bytes_per_rank"] == want
    assert d["weight_bytes_per_rank"] == 2 * (2 * linears + 2 * ln) + ln
    kv = d["kv_bytes_read_per_step_mean"]
    assert d["achieved_GBps"] == pytest.approx(
        (want + kv) / (d["ms_per_token_mean"] * 1e-3) / 1e9)
