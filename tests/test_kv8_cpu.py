"""FP8 (e4m3) KV cache, CPU side (torch path; gloo world 1): the cache's storage, the torch
append + decode against attention over ``_quantize_torch``'s dequantised rows, the model's decode
with the knob, config validation, and the ``run_tp --kv-cache`` record and refusals."""

import copy
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
from distributed_llm_backend_benchmark_amd.ops import decode as dec
from distributed_llm_backend_benchmark_amd.ops.fp8 import E4M3, _quantize_torch
from distributed_llm_backend_benchmark_amd.parallel.comm import Comm
from distributed_llm_backend_benchmark_amd.utils.config import (DEFAULT_CONFIG, ConfigError,
                                                                validate_config)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def test_kv_cache_fp8_storage():
    c = ops.KVCache(2, 2, 4, 64, 20, "cpu", kv_dtype="fp8")
    assert c.kv_dtype == "fp8" and len(c.k) == len(c.v) == len(c.k_scale) == len(c.v_scale) == 2
    for codes, scale in zip(c.k + c.v, c.k_scale + c.v_scale):
        assert codes.shape == (2, 4, 20, 64) and codes.dtype == E4M3 and codes.is_contiguous()
        assert scale.shape == (2, 4, 20) and scale.dtype == torch.float32
        assert scale.is_contiguous()
    assert c.nbytes == 2 * 2 * 2 * 4 * 20 * (64 + 4)
    assert c.workspace.numel() == dec.workspace_numel(2, 4, 64, 20, dec.CHUNK_FP8)
    plain = ops.KVCache(2, 2, 4, 64, 20, "cpu")
    assert plain.kv_dtype == "bf16" and plain.k_scale == [None, None] == plain.v_scale
    assert plain.nbytes == 2 * 2 * 2 * 4 * 20 * 64 * 2
    assert ops.KVCache(0, 2, 4, 64, 20, "cpu", kv_dtype="fp8").nbytes == 0
    with pytest.raises(ValueError):
        ops.KVCache(2, 2, 4, 64, 20, "cpu", kv_dtype="int8")
    assert dec.CHUNK_FP8 in (256, 512, 1024) and ops.CHUNK_FP8 == dec.CHUNK_FP8


def _rows(qkv, H, which):
    B, T, C3 = qkv.shape
    return qkv.view(B, T, 3, H, C3 // 3 // H)[:, :, which].permute(0, 2, 1, 3)   # [B, H, T, D]


@pytest.mark.parametrize("D", [32, 64, 128])
def test_torch_append_and_decode_equal_attention_over_the_quantised_rows(D):
    """Prefill append of 9 tokens, then 3 decode steps: the cache holds ``_quantize_torch``'s bits
    and every step equals SDPA over the dequantised rows (the new token's included), exactly."""
    B, H, T, L_max = 2, 3, 9, 14
    g = torch.Generator().manual_seed(D)
    qkv = torch.randn(B, T + 3, 3 * H * D, generator=g).to(BF16)
    qkv[0, 2, H * D:H * D + D] = 0                      # an all-zero K row: scale 1, codes 0
    kc, vc = (torch.full((B, H, L_max, D), 0x7F, dtype=torch.uint8).view(E4M3) for _ in range(2))
    ks, vs = (torch.full((B, H, L_max), float("nan")) for _ in range(2))
    length = torch.zeros(1, dtype=torch.int32)
    ops.kv_append(qkv[:, :T].contiguous(), H, kc, vc, length, pos=0, k_scale=ks, v_scale=vs)
    length.fill_(T)
    for t in range(T, T + 3):
        step = qkv[:, t:t + 1].contiguous()
        got = ops.decode_attention(step, H, kc, vc, length, pos=t, k_scale=ks, v_scale=vs)
        length.add_(1)
        kq, ksc = _quantize_torch(_rows(qkv[:, :t + 1], H, 1))
        vq, vsc = _quantize_torch(_rows(qkv[:, :t + 1], H, 2))
        assert torch.equal(kc.view(torch.uint8)[:, :, :t + 1], kq.view(torch.uint8))
        assert torch.equal(vc.view(torch.uint8)[:, :, :t + 1], vq.view(torch.uint8))
        assert torch.equal(ks[:, :, :t + 1], ksc) and torch.equal(vs[:, :, :t + 1], vsc)
        assert (kc.view(torch.uint8)[:, :, t + 1:] == 0x7F).all() and ks[:, :, t + 1:].isnan().all()
        q = _rows(step, H, 0).float()
        want = torch.nn.functional.scaled_dot_product_attention(
            q, kq.float() * ksc[..., None], vq.float() * vsc[..., None]).to(BF16)
        assert torch.equal(got, want.transpose(1, 2).reshape(B, 1, H * D))
    assert float(ks[0, 0, 2]) == 1.0 and not kc.view(torch.uint8)[0, 0, 2].any()
    with pytest.raises(ValueError):                      # host overflow check
        ops.kv_append(qkv[:, :T].contiguous(), H, kc, vc, length, pos=L_max - T + 1, k_scale=ks,
                      v_scale=vs)
    with pytest.raises(ValueError):                      # an e4m3 cache without its scales
        ops.decode_attention(qkv[:, :1].contiguous(), H, kc, vc, length, pos=0)
    with pytest.raises(ValueError):                      # scales with a bf16 cache
        ops.decode_attention(qkv[:, :1].contiguous(), H, kc.float().to(BF16), vc.float().to(BF16),
                             length, pos=0, k_scale=ks, v_scale=vs)


def _model(**kw):
    comm = Comm(0, 1, 0, "gloo", torch.device("cpu"))
    return LLM(hidden_size=256, num_layers=2, num_heads=4, ffn_intermediate=1024, comm=comm,
               seed=3, init_std=0.05, kernels="torch", attention="sdpa", **kw)


def _decode(model, x, prompt):
    cache = model.new_kv_cache(x.shape[0], x.shape[1])
    rows = [model(x[:, :prompt].contiguous(), kv_cache=cache)]
    rows += [model(x[:, t:t + 1].contiguous(), kv_cache=cache) for t in range(prompt, x.shape[1])]
    return torch.cat(rows, 1).float(), cache


def test_model_decode_with_the_fp8_cache():
    """The project's TP-vs-dense bound 3e-2 of max|ref| against the full forward's rows; the
    steps read e4m3 rows, so they are not the bf16-cache steps' bits."""
    model = _model(kv_cache_dtype="fp8")
    assert model.kv_cache_dtype == "fp8" and _model().kv_cache_dtype == "bf16"
    x = torch.randn(2, 24, 256, generator=torch.Generator().manual_seed(7)).to(BF16)
    ref = model(x).float()
    got, cache = _decode(model, x, 16)
    assert cache.kv_dtype == "fp8" and cache.k[0].dtype == E4M3 and cache.pos == 24
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"fp8-cache decode vs the full forward: {err:.3e}")
    assert err < 3e-2, err
    plain = _model()
    plain.load_state_dict(model.state_dict())
    base, cache = _decode(plain, x, 16)
    assert cache.kv_dtype == "bf16" and cache.k[0].dtype == BF16
    assert torch.equal(got[:, :16], base[:, :16])       # the prefill is unchanged
    dist = float((got[:, 16:] - base[:, 16:]).abs().max() / base.abs().max())
    print(f"fp8-cache decode vs bf16-cache decode: {dist:.3e}")
    assert 0 < dist < 3e-2
    with pytest.raises(ValueError):
        _model(kv_cache_dtype="int8")


def test_config_validation():
    cfg = validate_config(copy.deepcopy(DEFAULT_CONFIG))
    assert cfg["execution"]["kv_cache_dtype"] == "bf16"
    raw = copy.deepcopy(DEFAULT_CONFIG)
    del raw["execution"]["kv_cache_dtype"]
    assert validate_config(raw)["execution"]["kv_cache_dtype"] == "bf16"
    raw["execution"]["kv_cache_dtype"] = "fp8"
    assert validate_config(raw)["execution"]["kv_cache_dtype"] == "fp8"
    raw["execution"]["kv_cache_dtype"] = "int8"
    with pytest.raises(ConfigError, match="kv_cache_dtype"):
        validate_config(raw)


def _run_tp(cfg_path, *extra):
    return subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                           "--config", str(cfg_path), "--backend", "gloo", "--device", "cpu",
                           *extra], capture_output=True, text=True, timeout=600, cwd=REPO)


def test_run_tp_kv_cache_record_on_cpu(tmp_path):
    import yaml

    from distributed_llm_backend_benchmark_amd.cli import run_tp

    assert run_tp.parse_args(["--config", "c.yaml"]).kv_cache is None
    cfg = yaml.safe_load(open(os.path.join(REPO, "config", "baseline_config.yaml")))
    cfg["model"].update(hidden_size=64, num_layers=2, num_heads=2, ffn_intermediate=128,
                        init_std=0.05)
    cfg["input"].update(batch_size=2, sequence_length=16)
    cfg["execution"].update(warmup_iterations=1, benchmark_iterations=2, attention="sdpa",
                            kernels="torch")
    cfg["parallelism"]["world_size"] = 1
    cfg["experiment"]["output_dir"] = str(tmp_path)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    name = cfg["experiment"]["name"]

    for refused in (["--kv-cache", "fp8"],                                     # no decode tokens
                    ["--decode", "4", "--kv-cache", "fp8", "--attention", "slice"]):
        out = _run_tp(p, *refused)
        assert out.returncode == 1 and "ERROR" in out.stdout, out.stderr[-3000:]
        assert not [f for f in os.listdir(tmp_path) if f.endswith(".json")]

    out = _run_tp(p, "--decode", "4", "--kv-cache", "fp8")
    assert out.returncode == 0, out.stderr[-3000:]
    assert not (tmp_path / f"gloo_{name}_decode4.json").exists()
    rec = json.load(open(tmp_path / f"gloo_{name}_decode4_kv8.json"))
    d = rec["decode"]
    assert rec["config"]["execution"]["kv_cache_dtype"] == "fp8"
    assert d["kv_dtype"] == "fp8" and d["weight_dtype"] == "bf16"
    # 2 layers x (K, V) x 2 entries x 2 heads x 20 positions x (32 codes + one fp32 scale)
    assert d["kv_cache_bytes_per_rank"] == 2 * 2 * 2 * 2 * 20 * (32 + 4)
    # steps read 17, 18, 19, 20 keys
    assert d["kv_bytes_read_per_step_mean"] == 18.5 * 2 * 2 * 2 * 2 * (32 + 4)
    assert d["achieved_GBps"] == pytest.approx(
        (d["weight_bytes_per_rank"] + d["kv_bytes_read_per_step_mean"])
        / (d["ms_per_token_mean"] * 1e-3) / 1e9)

    out = _run_tp(p, "--decode", "4", "--decode-weights", "fp8", "--kv-cache", "fp8")
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.load(open(tmp_path / f"gloo_{name}_decode4_w8_kv8.json"))["decode"]
    assert d["kv_dtype"] == "fp8" and d["weight_dtype"] == "fp8"

    out = _run_tp(p, "--decode", "4")
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.load(open(tmp_path / f"gloo_{name}_decode4.json"))["decode"]
    assert d["kv_dtype"] == "bf16"
    assert d["kv_cache_bytes_per_rank"] == 2 * 2 * 2 * 2 * 20 * 32 * 2
