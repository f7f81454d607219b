"""Decode over a batch of sequences with different lengths, CPU side (torch path; gloo world 1):
the per-sequence ``KVCache`` bookkeeping, ragged append / decode against a per-row loop of the
shared-length torch forms on batch-1 slices (bit for bit), the ``length.numel()`` dispatch, the
model's padded prefill + decode + retire-and-refill against batch-1 runs, and the ``run_tp
--prompt-lens`` argument errors."""

import os
import subprocess
import sys

import pytest
import torch

from distributed_llm_backend_benchmark_amd import ops
from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
from distributed_llm_backend_benchmark_amd.ops import decode as dec
from distributed_llm_backend_benchmark_amd.ops.fp8 import E4M3
from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = torch.int32


def test_per_sequence_bookkeeping():
    c = ops.KVCache(2, 3, 4, 64, 20, "cpu", per_sequence=True)
    assert c.per_sequence and c.length.shape == (3,) and c.length.dtype == I32
    assert c.pos == [0, 0, 0] and c.length.tolist() == [0, 0, 0]
    assert c.nbytes == 2 * 2 * 3 * 4 * 20 * 64 * 2                # as the shared-length cache
    assert c.live_bytes() == 0
    c.set_lengths([3, 7, 5])
    assert c.pos == [3, 7, 5] and c.length.tolist() == [3, 7, 5]
    assert c.live_bytes() == (3 + 7 + 5) * 2 * 4 * 64 * 2 * 2     # layers x heads x D bf16, K + V
    c.retire(1)
    assert c.pos == [3, -1, 5] and c.length.tolist() == [3, -1, 5]
    c.advance(2)                                                  # the retired row stays at -1
    assert c.pos == [5, -1, 7] and c.length.tolist() == [5, -1, 7]
    assert c.live_bytes() == (5 + 7) * 2 * 4 * 64 * 2 * 2
    c.check_room(13)                                              # the longest live row: 7 + 13
    with pytest.raises(ValueError):
        c.check_room(14)
    with pytest.raises(ValueError):
        c.advance(14)
    assert c.pos == [5, -1, 7] and c.length.tolist() == [5, -1, 7]    # a refused advance: nothing
    with pytest.raises(ValueError):
        c.set_lengths([1, 2])                                     # one value per row
    with pytest.raises(ValueError):
        c.set_lengths([1, 2, 21])
    c.set_length(0)                                               # every row
    assert c.pos == [0, 0, 0] and c.length.tolist() == [0, 0, 0]


def test_default_cache_is_the_shared_length_one():
    c = ops.KVCache(1, 3, 2, 64, 8, "cpu")
    assert not c.per_sequence and c.length.shape == (1,) and c.pos == 0
    for call in (lambda: c.set_lengths([1, 1, 1]), lambda: c.retire(0), lambda: c.slot(0)):
        with pytest.raises(ValueError):
            call()
    c.set_length(3)
    assert c.live_bytes() == 3 * 3 * 2 * 64 * 2 * 2


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_slot_shares_storage_and_mirrors_pos(kv_dtype):
    c = ops.KVCache(2, 3, 2, 64, 10, "cpu", kv_dtype=kv_dtype, per_sequence=True)
    c.set_lengths([4, -1, 6])
    s = c.slot(1)
    assert s.batch == 1 and not s.per_sequence and s.pos == -1 and s.length.shape == (1,)
    assert s.kv_dtype == kv_dtype and s.workspace is c.workspace
    for mine, theirs in zip(s.k + s.v, c.k + c.v):
        assert mine.shape == (1, 2, 10, 64) and mine.is_contiguous()
        assert mine.data_ptr() == theirs[1].data_ptr()
    if kv_dtype == "fp8":
        assert s.k_scale[1].data_ptr() == c.k_scale[1][1].data_ptr()
        assert c.live_bytes() == (4 + 6) * 2 * 2 * (64 + 4) * 2
    else:
        assert s.k_scale == [None, None]
    assert s.length.data_ptr() == c.length[1:].data_ptr()
    s.set_length(0)
    assert c.pos == [4, 0, 6] and c.length.tolist() == [4, 0, 6]
    s.advance(5)
    assert s.pos == 5 and c.pos == [4, 5, 6] and c.length.tolist() == [4, 5, 6]
    s.k[0].view(torch.uint8)[0, 1, 2, 3] = 77
    assert int(c.k[0].view(torch.uint8)[1, 1, 2, 3]) == 77
    with pytest.raises(ValueError):
        c.slot(3)


def _filled(kv_dtype, B, H, D, L_max, seed):
    """A per-sequence cache of one layer holding random rows everywhere (appended as one block
    from position 0), and a clone of its tensors for the per-row reference."""
    g = torch.Generator().manual_seed(seed)
    c = ops.KVCache(1, B, H, D, L_max, "cpu", kv_dtype=kv_dtype, per_sequence=True)
    fill = torch.randn(B, L_max, 3 * H * D, generator=g).to(torch.bfloat16)
    dec.kv_append(fill, H, c.k[0], c.v[0], c.length, pos=c.pos, k_scale=c.k_scale[0],
                  v_scale=c.v_scale[0])
    return c, g


def _tensors(c):
    return [t for t in (c.k[0], c.v[0], c.k_scale[0], c.v_scale[0]) if t is not None]


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _row_ref(fn, qkv, H, ref, lens, b):
    """The shared-length torch form on the batch-1 slice of row ``b`` of the cloned tensors."""
    k, v = ref[0][b:b + 1], ref[1][b:b + 1]
    ks, vs = (ref[2][b:b + 1], ref[3][b:b + 1]) if len(ref) == 4 else (None, None)
    return fn(qkv[b:b + 1], H, k, v, lens[b], ks, vs)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("T", [1, 5])
def test_ragged_append_equals_the_per_row_loop(kv_dtype, D, T):
    B, H, L_max, lens = 4, 2, 24, [-1, 0, 7, 19]
    c, g = _filled(kv_dtype, B, H, D, L_max, seed=D + T)
    ref = [t.clone() for t in _tensors(c)]
    before = [t.clone() for t in ref]
    c.set_lengths(lens)
    qkv = torch.randn(B, T, 3 * H * D, generator=g).to(torch.bfloat16)
    dec.kv_append(qkv, H, c.k[0], c.v[0], c.length, pos=c.pos, k_scale=c.k_scale[0],
                  v_scale=c.v_scale[0])
    for b in range(1, B):
        _row_ref(dec.torch_kv_append, qkv, H, ref, lens, b)
    for got, want, old in zip(_tensors(c), ref, before):
        assert torch.equal(_bits(got), _bits(want))
        assert torch.equal(_bits(got[0]), _bits(old[0]))          # the empty slot: untouched
        assert not torch.equal(_bits(got[2]), _bits(old[2]))
    # the device lengths alone (pos=None) give the same cache
    c2, _ = _filled(kv_dtype, B, H, D, L_max, seed=D + T)
    c2.set_lengths(lens)
    dec.kv_append(qkv, H, c2.k[0], c2.v[0], c2.length, k_scale=c2.k_scale[0],
                  v_scale=c2.v_scale[0])
    for got, want in zip(_tensors(c2), ref):
        assert torch.equal(_bits(got), _bits(want))
    with pytest.raises(ValueError):                               # the longest row overflows
        dec.kv_append(qkv, H, c.k[0], c.v[0], c.length, pos=[-1, 0, 7, L_max - T + 1],
                      k_scale=c.k_scale[0], v_scale=c.v_scale[0])


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("D", [32, 64])
def test_ragged_decode_equals_the_per_row_loop(kv_dtype, D):
    B, H, L_max, lens = 5, 2, 24, [-1, 0, 7, 19, 23]
    c, g = _filled(kv_dtype, B, H, D, L_max, seed=3 * D)
    ref = [t.clone() for t in _tensors(c)]
    c.set_lengths(lens)
    qkv = torch.randn(B, 1, 3 * H * D, generator=g).to(torch.bfloat16)
    got = dec.decode_attention(qkv, H, c.k[0], c.v[0], c.length, pos=c.pos,
                               k_scale=c.k_scale[0], v_scale=c.v_scale[0])
    assert got.shape == (B, 1, H * D) and got.dtype == torch.bfloat16
    assert not _bits(got[0]).any()                                # the empty slot: zero bits
    for b in range(1, B):
        want = _row_ref(dec.torch_decode_attention, qkv, H, ref, lens, b)
        assert torch.equal(_bits(got[b:b + 1]), _bits(want)), b
        assert bool(want.float().abs().max() > 0)
    for mine, theirs in zip(_tensors(c), ref):                    # the appended tokens too
        assert torch.equal(_bits(mine), _bits(theirs))
    assert c.length.tolist() == lens                              # not advanced
    again = dec.decode_attention(qkv, H, c.k[0], c.v[0], c.length, k_scale=c.k_scale[0],
                                 v_scale=c.v_scale[0])            # positions from the device
    assert torch.equal(_bits(again), _bits(got))


@pytest.mark.parametrize("n", [0, 2, 4])
def test_length_numel_must_be_1_or_the_batch(n):
    B, H, D, L_max = 3, 2, 32, 8
    qkv = torch.zeros(B, 1, 3 * H * D, dtype=torch.bfloat16)
    kc = torch.zeros(B, H, L_max, D, dtype=torch.bfloat16)
    vc = torch.zeros_like(kc)
    length = torch.zeros(n, dtype=I32)
    with pytest.raises(ValueError):
        dec.kv_append(qkv, H, kc, vc, length)
    with pytest.raises(ValueError):
        dec.decode_attention(qkv, H, kc, vc, length)
    codes = torch.zeros(B, H, L_max, D, dtype=E4M3)
    scales = torch.ones(B, H, L_max)
    with pytest.raises(ValueError):
        dec.decode_attention(qkv, H, codes, codes.clone(), length, k_scale=scales,
                             v_scale=scales.clone())


def _model():
    comm = Comm(0, 1, 0, "gloo", torch.device("cpu"))
    return LLM(hidden_size=256, num_layers=2, num_heads=4, ffn_intermediate=1024, comm=comm,
               seed=3, init_std=0.05, kernels="torch", attention="sdpa")


def _single(m, prompt, steps, max_len):
    """A batch-1 run on a shared-length cache: the prefill output at the last prompt token, then
    ``steps`` decode steps, each fed the previous output -> [1 + steps, hidden] fp32."""
    cache = m.new_kv_cache(1, max_len)
    y = m(prompt[None].contiguous(), kv_cache=cache)[:, -1:]
    rows = [y]
    for _ in range(steps):
        rows.append(m(rows[-1], kv_cache=cache))
    return torch.cat(rows, dim=1)[0].float()


def _close(got, want, scale, what):
    """The dense comparison's tolerance of tests/test_decode_cpu.py: 3e-2 of max|ref|."""
    err = float((got.float() - want).abs().max()) / scale
    assert err < 3e-2, (what, err)


def test_model_ragged_prefill_decode_retire_and_refill():
    m = _model()
    lens, S, steps, max_len = [3, 7, 5], 7, 4, 16
    g = torch.Generator().manual_seed(7)
    x = torch.randn(3, S, 256, generator=g).to(torch.bfloat16)
    for b, n in enumerate(lens):
        x[b, n:] = 100.0                                          # padding the model must not see
    refs = [_single(m, x[b, :n], steps + 1, max_len) for b, n in enumerate(lens)]
    scale = max(float(r.abs().max()) for r in refs)

    cache = m.new_kv_cache(3, max_len, per_sequence=True)
    y = m(x, kv_cache=cache, prompt_lens=lens)
    assert cache.pos == lens and cache.length.tolist() == lens
    tok = torch.stack([y[b, n - 1] for b, n in enumerate(lens)])[:, None]
    for b in range(3):
        _close(tok[b, 0], refs[b][0], scale, ("prefill", b))
    for i in range(steps):
        tok = m(tok, kv_cache=cache)
        for b in range(3):
            _close(tok[b, 0], refs[b][1 + i], scale, ("step", i, b))
    assert cache.pos == [n + steps for n in lens]

    # a twin that never touches slot 1, from the same state
    twin = m.new_kv_cache(3, max_len, per_sequence=True)
    for mine, theirs in zip(twin.k + twin.v, cache.k + cache.v):
        mine.copy_(theirs)
    twin.set_lengths(cache.pos)
    twin.retire(1)
    twin_out = m(tok, kv_cache=twin)

    cache.retire(1)
    new = torch.randn(4, 256, generator=g).to(torch.bfloat16)
    fresh = _single(m, new, 1, max_len)
    slot = cache.slot(1)
    with pytest.raises(ValueError):
        m(new[None], kv_cache=slot)                               # a retired row is claimed first
    slot.set_length(0)
    y1 = m(new[None].contiguous(), kv_cache=slot)
    assert cache.pos == [lens[0] + steps, 4, lens[2] + steps]
    assert cache.length.tolist() == cache.pos
    _close(y1[0, -1], fresh[0], scale, "refill prefill")
    tok = torch.cat([tok[0:1], y1[:, -1:], tok[2:3]])
    out = m(tok, kv_cache=cache)
    for b in (0, 2):                                              # as if slot 1 was never touched
        assert torch.equal(out[b], twin_out[b]), b
        _close(out[b, 0], refs[b][1 + steps], scale, ("after refill", b))
    _close(out[1, 0], fresh[1], scale, "refilled row")
    assert cache.pos == [lens[0] + steps + 1, 5, lens[2] + steps + 1]


def test_forward_refuses_bad_prompt_lens():
    m = _model()
    x = torch.zeros(3, 7, 256, dtype=torch.bfloat16)
    cache = m.new_kv_cache(3, 16, per_sequence=True)
    for bad in ([3, 7], [0, 7, 5], [3, 8, 5]):
        with pytest.raises(ValueError):
            m(x, kv_cache=cache, prompt_lens=bad)
    assert cache.pos == [0, 0, 0]
    with pytest.raises(ValueError):
        m(x, kv_cache=m.new_kv_cache(3, 16), prompt_lens=[3, 7, 5])      # a shared-length cache
    m(x, kv_cache=cache, prompt_lens=[3, 7, 5])
    with pytest.raises(ValueError):
        m(x, kv_cache=cache, prompt_lens=[3, 7, 5])               # live rows are not empty
    with pytest.raises(ValueError):
        m(x[:, :1], kv_cache=cache, prompt_lens=[1, 1, 1])        # a decode step takes none


def _cfg(tmp_path):
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
    return p


@pytest.mark.parametrize("extra", [["--prompt-lens", "5,16"],
                                   ["--decode", "4", "--prompt-lens", "5,9,16"],
                                   ["--decode", "4", "--prompt-lens", "0,16"],
                                   ["--decode", "4", "--prompt-lens", "5,17"]])
def test_run_tp_prompt_lens_argument_errors(tmp_path, extra):
    """No ``--decode``, a wrong count, a value below 1 and one above ``sequence_length``: exit code
    1, ERROR, no JSON."""
    from distributed_llm_backend_benchmark_amd.cli import run_tp

    assert run_tp.parse_args(["--config", "c.yaml", "--prompt-lens", "5,16"]).prompt_lens == "5,16"
    out = subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                          "--config", str(_cfg(tmp_path)), "--backend", "gloo", "--device", "cpu",
                          *extra], capture_output=True, text=True, timeout=600, cwd=REPO)
    assert out.returncode == 1 and "ERROR" in out.stdout and "prompt" in out.stdout, \
        out.stderr[-3000:]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".json")]


def test_config_accepts_prompt_lengths_and_has_no_default():
    import copy

    from distributed_llm_backend_benchmark_amd.utils.config import (DEFAULT_CONFIG, ConfigError,
                                                                    validate_config)

    cfg = copy.deepcopy(DEFAULT_CONFIG)
    assert "prompt_lengths" not in validate_config(cfg)["execution"]
    B, S = cfg["input"]["batch_size"], cfg["input"]["sequence_length"]
    cfg["execution"]["prompt_lengths"] = [S] * B
    assert validate_config(cfg)["execution"]["prompt_lengths"] == [S] * B
    for bad in ([S] * (B + 1), [0] + [S] * (B - 1), [S + 1] * B, "3"):
        cfg["execution"]["prompt_lengths"] = bad
        with pytest.raises(ConfigError):
            validate_config(cfg)
