"""Decode through the tensor-parallel model on the GPU: prefill + teacher-forced decode steps
equal the full causal forward's rows (world 1, and P = 2 with both ranks on one GPU), every
decode step runs the HIP decode kernel, and ``run_tp --decode`` writes its record."""

import json
import os
import subprocess
import sys

import pytest
import torch

from mp_utils import run_multiprocess

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(hidden_size=256, num_layers=2, ffn_intermediate=1024, seed=11, init_std=0.05,
          attention="flash")


def _input(dev, tokens=64):
    g = torch.Generator(device=dev).manual_seed(5)
    return torch.randn(2, tokens, 256, generator=g, device=dev).to(torch.bfloat16)


def _decode_rows(model, x, prompt):
    """Prefill ``x[:, :prompt]`` then teacher-forced steps; returns all output rows [B, T, H]."""
    cache = model.new_kv_cache(x.shape[0], x.shape[1])
    rows = [model(x[:, :prompt].contiguous(), kv_cache=cache)]
    for t in range(prompt, x.shape[1]):
        rows.append(model(x[:, t:t + 1].contiguous(), kv_cache=cache))
    assert cache.pos == x.shape[1] and int(cache.length) == x.shape[1]
    return torch.cat(rows, dim=1).float()


@pytest.mark.parametrize("heads", [4, 2])
def test_decode_equals_full_flash_forward_world1(heads):
    """Head dim 64 (4 heads) and 128 (2 heads): 48 prompt tokens + 16 decode steps against the
    full 64-token forward, both on ``flash`` — only the decode path differs. Bound 3e-2 of
    max|ref| (the project's TP-vs-dense bound)."""
    from distributed_llm_backend_benchmark_amd import ops as O
    from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
    from distributed_llm_backend_benchmark_amd.ops import decode as dec
    from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

    dev = torch.device("cuda", 0)
    model = LLM(comm=Comm(0, 1, 0, "gloo", dev), num_heads=heads, **KW)
    x = _input(dev)
    ref = model(x).float()
    calls = [0, 0]
    real = O.decode_attention

    def counted(qkv, n_head, k_cache, v_cache, length, **kw):
        calls[0] += 1
        calls[1] += int(dec.use_hip(qkv) and dec.hip_supported(qkv, n_head, k_cache, v_cache))
        return real(qkv, n_head, k_cache, v_cache, length, **kw)

    O.decode_attention = counted
    try:
        got = _decode_rows(model, x, 48)
    finally:
        O.decode_attention = real
    torch.cuda.synchronize()
    assert calls == [16 * 2, 16 * 2], calls            # every step of every layer, on the kernel
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"decode vs full forward, heads={heads}: {err:.3e}")
    assert err < 3e-2, err


def _tp_decode_worker(rank, world, heads):
    from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
    from distributed_llm_backend_benchmark_amd.parallel.comm import Comm, init_distributed

    comm = init_distributed("gloo", device="cuda")
    dev = comm.device
    dense = LLM(comm=Comm(0, 1, 0, "gloo", dev), num_heads=heads, **KW)
    tp = LLM(comm=comm, num_heads=heads, allreduce="rccl", **KW)
    tp.load_from_dense(dense.state_dict())
    x = _input(dev, 56)
    ref = dense(x).float()
    got = _decode_rows(tp, x, 48)
    torch.cuda.synchronize()
    err = float((got - ref).abs().max() / ref.abs().max())
    comm.destroy()
    return err


@pytest.mark.parametrize("heads", [4, 2])
def test_tp_decode_ranks_on_one_gpu_matches_dense(heads):
    """P = 2 over gloo on one GPU: prefill + 8 decode steps of the sharded model (2 / 1 local
    heads) equal the dense world-1 model's full forward rows."""
    errs = run_multiprocess(_tp_decode_worker, 2, args=(heads,), timeout=600)
    assert max(errs) < 3e-2, errs


def _cfg(tmp_path, world=1):
    import yaml

    cfg = yaml.safe_load(open(os.path.join(REPO, "config", "baseline_config.yaml")))
    cfg["model"].update(hidden_size=512, num_layers=2, num_heads=8, ffn_intermediate=2048,
                        init_std=0.02)
    cfg["input"].update(batch_size=2, sequence_length=64)
    cfg["execution"].update(warmup_iterations=1, benchmark_iterations=3)
    cfg["parallelism"]["world_size"] = world
    cfg["experiment"]["output_dir"] = str(tmp_path)
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return p, cfg["experiment"]["name"]


def _run_tp(cfg_path, *extra):
    return subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                           "--config", str(cfg_path), "--backend", "rccl", *extra],
                          capture_output=True, text=True, timeout=600, cwd=REPO)


@pytest.mark.parametrize("eager", [False, True])
def test_run_tp_decode_flash(tmp_path, eager):
    p, name = _cfg(tmp_path)
    out = _run_tp(p, "--decode", "8", "--attention", "flash", *(["--eager"] if eager else []))
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.load(open(tmp_path / f"rccl_{name}_decode8.json"))
    d = rec["decode"]
    assert d["timing_mode"] == ("eager" if eager else "hip_graph_replay"), d["hip_graph_note"]
    assert d["attention_path"] == "hip"
    assert len(d["ms_per_token"]) == 3 and all(v > 0 for v in d["ms_per_token"])
    assert (d["prompt_len"], d["new_tokens"], d["max_len"]) == (64, 8, 72)
    assert d["kv_cache_bytes_per_rank"] == 2 * 2 * 2 * 8 * 72 * 64 * 2
    assert len(rec["raw_metrics_rank_0"]["forward_times"]) == 3
    assert not (tmp_path / f"rccl_{name}.json").exists()


def test_run_tp_decode_shard_as(tmp_path):
    p, name = _cfg(tmp_path, world=4)
    out = _run_tp(p, "--decode", "4", "--attention", "flash", "--shard-as", "4")
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.load(open(tmp_path / f"rccl_{name}_shard4_decode4.json"))
    assert rec["decode"]["attention_path"] == "hip"
    assert rec["decode"]["allreduce_bytes_per_step"] == 2 * 2 * 2 * 512 * 2
    assert rec["throughput"]["shard_as"]["P"] == 4


def test_run_tp_decode_refuses_fp8(tmp_path):
    p, name = _cfg(tmp_path)
    out = _run_tp(p, "--decode", "4", "--gemm-dtype", "fp8")
    assert out.returncode == 1 and "fp8" in out.stdout
    assert not list(tmp_path.glob("*.json"))
