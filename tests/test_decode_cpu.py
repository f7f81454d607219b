"""Token-by-token decode with a KV cache, CPU side (torch path; gloo world 1): cache
bookkeeping, decode == the full causal forward's rows, config / CLI plumbing, and the
``run_tp --decode`` record."""

import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECODE_KEYS = {"prompt_len", "new_tokens", "max_len", "ms_per_token", "ms_per_token_mean",
               "ms_per_token_p50", "decode_tokens_per_s", "kv_cache_bytes_per_rank",
               "kv_bytes_read_per_step_mean", "weight_bytes_per_rank", "achieved_GBps",
               "allreduce_bytes_per_step", "attention_path", "timing_mode", "gemm_kernel_mix"}


def _model(attention):
    comm = Comm(0, 1, 0, "gloo", torch.device("cpu"))
    return LLM(hidden_size=256, num_layers=2, num_heads=4, ffn_intermediate=1024, comm=comm,
               seed=3, init_std=0.05, kernels="torch", attention=attention)


def _x():
    g = torch.Generator().manual_seed(7)
    return torch.randn(2, 24, 256, generator=g).to(torch.bfloat16)


def test_kv_cache_bookkeeping():
    c = ops.KVCache(2, 2, 4, 64, 20, "cpu")
    assert c.k[0].shape == (2, 4, 20, 64) and c.k[0].dtype == torch.bfloat16
    assert c.nbytes == 2 * 2 * 2 * 4 * 20 * 64 * 2
    assert c.pos == 0 and int(c.length) == 0 and c.length.dtype == torch.int32
    c.set_length(5)
    assert c.pos == 5 and int(c.length) == 5
    c.advance(3)
    assert c.pos == 8 and int(c.length) == 8
    c.advance(12)
    assert c.pos == 20
    with pytest.raises(ValueError):
        c.advance(1)
    assert c.pos == 20 and int(c.length) == 20          # a refused advance changes nothing
    with pytest.raises(ValueError):
        c.set_length(21)
    c.set_length(0)
    assert c.pos == 0 and int(c.length) == 0


def test_forward_refuses_overflow_and_chunked_prefill():
    m = _model("sdpa")
    x = _x()
    cache = m.new_kv_cache(2, 20)
    with pytest.raises(ValueError):
        m(x, kv_cache=cache)                             # 24 tokens > max_len 20
    assert cache.pos == 0
    m(x[:, :16], kv_cache=cache)
    assert cache.pos == 16 and int(cache.length) == 16
    with pytest.raises(ValueError):
        m(x[:, 16:20], kv_cache=cache)                   # T > 1 on a non-empty cache
    for i in range(4):
        m(x[:, 16 + i:17 + i], kv_cache=cache)
    assert cache.pos == 20
    with pytest.raises(ValueError):
        m(x[:, 20:21], kv_cache=cache)                   # pos + 1 > max_len


@pytest.mark.parametrize("attention", ["sdpa", "slice"])
def test_decode_equals_full_forward_rows(attention):
    """Prefill 16 tokens, then 8 teacher-forced decode steps: every step's output is row 16 + i
    of the full causal forward on all 24 tokens (bound: the project's TP-vs-dense 3e-2)."""
    m = _model(attention)
    x = _x()
    ref = m(x).float()
    scale = float(ref.abs().max())
    cache = m.new_kv_cache(2, 24)
    assert (cache.num_layers == 0 and cache.nbytes == 0) if attention == "slice" \
        else cache.num_layers == 2
    y = m(x[:, :16], kv_cache=cache).float()
    assert float((y - ref[:, :16]).abs().max()) / scale < 3e-2
    for i in range(8):
        y = m(x[:, 16 + i:17 + i], kv_cache=cache).float()
        assert y.shape == (2, 1, 256)
        err = float((y[:, 0] - ref[:, 16 + i]).abs().max()) / scale
        assert err < 3e-2, (i, err)
    assert cache.pos == 24 and int(cache.length) == 24


def test_config_and_cli_accept_decode():
    import copy

    from distributed_llm_backend_benchmark_amd.cli import run_tp
    from distributed_llm_backend_benchmark_amd.utils.config import (DEFAULT_CONFIG, ConfigError,
                                                                    validate_config)

    cfg = copy.deepcopy(DEFAULT_CONFIG)
    assert validate_config(cfg)["execution"]["decode_tokens"] == 0
    cfg["execution"].update(attention="flash", decode_tokens=8)
    out = validate_config(cfg)
    assert out["execution"]["attention"] == "flash" and out["execution"]["decode_tokens"] == 8
    cfg["execution"]["decode_tokens"] = -1
    with pytest.raises(ConfigError):
        validate_config(cfg)
    a = run_tp.parse_args(["--config", "c.yaml", "--decode", "5", "--max-len", "99"])
    assert a.decode == 5 and a.max_len == 99
    assert run_tp.parse_args(["--config", "c.yaml"]).decode is None


def _run_tp(cfg_path, *extra):
    return subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                           "--config", str(cfg_path), "--backend", "gloo", "--device", "cpu",
                           *extra], capture_output=True, text=True, timeout=600, cwd=REPO)


def test_run_tp_decode_record_on_cpu(tmp_path):
    import yaml

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

    out = _run_tp(p, "--decode", "4")
    assert out.returncode == 0, out.stderr[-3000:]
    assert not (tmp_path / f"gloo_{name}.json").exists()
    rec = json.load(open(tmp_path / f"gloo_{name}_decode4.json"))
    d = rec["decode"]
    assert DECODE_KEYS <= set(d), sorted(DECODE_KEYS - set(d))
    assert (d["prompt_len"], d["new_tokens"], d["max_len"]) == (16, 4, 20)
    assert len(d["ms_per_token"]) == 2 and all(v > 0 for v in d["ms_per_token"])
    assert d["attention_path"] == "torch" and d["timing_mode"] == "eager"
    assert d["kv_cache_bytes_per_rank"] == 2 * 2 * 2 * 2 * 20 * 32 * 2
    # steps read 17, 18, 19, 20 keys of 2 layers x 2 entries x 2 heads x 32 columns, K and V
    assert d["kv_bytes_read_per_step_mean"] == 18.5 * 2 * 2 * 2 * 32 * 2 * 2
    assert d["allreduce_bytes_per_step"] == 2 * 2 * 2 * 64 * 2
    assert len(rec["raw_metrics_rank_0"]["forward_times"]) == 2

    out = _run_tp(p)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.load(open(tmp_path / f"gloo_{name}.json"))
    assert "decode" not in rec

    out = _run_tp(p, "--decode", "4", "--gemm-dtype", "fp8")
    assert out.returncode == 1 and "fp8" in out.stdout
