"""The FP8 (e4m3) KV-cache kernels (csrc/attn_decode.hip) against an fp32 softmax over the
DEQUANTISED torch-quantised K / V (``ops.fp8._quantize_torch`` on the CPU), so both sides see the
same codes and scales: every key position, slot and chunk edges, the device-side length, bit-exact
quantising appends, determinism, HIP-graph replay across positions, the model's decode with
``kv_cache_dtype="fp8"`` and the ``run_tp --kv-cache fp8`` record."""

import json
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_llm_backend_benchmark_amd.ops import decode as dec
from distributed_llm_backend_benchmark_amd.ops.decode import (CHUNK_FP8, decode_attention,
                                                              kv_append)
from distributed_llm_backend_benchmark_amd.ops.fp8 import E4M3, _quantize_torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NAN = float("nan")
NAN_CODE = 0x7F                      # the e4m3fn NaN byte
U8 = torch.uint8
SLOTS = {64: 64, 128: 32}            # key slots per workgroup: 256 threads / (D / 16 lanes per key)


def _quant(x):
    """``_quantize_torch`` of CPU rows -> (code bytes uint8, fp32 scales), on the device."""
    code, scale = _quantize_torch(x.cpu())
    return code.view(U8).to(DEV), scale.to(DEV)


def _dequant(code, scale):
    return code.view(E4M3).float() * scale[..., None]


def _ref(q, K, V):
    """fp32 softmax attention of q [B, H, D] over fp32 K / V [B, H, L, D] -> fp32."""
    D = q.shape[-1]
    s = (q.float()[:, :, None, :] * K).sum(-1) / math.sqrt(D)                # [B, H, L]
    p = torch.softmax(s, dim=-1)
    return (p[..., None] * V).sum(2), s


def _pack(q, k_new, v_new):
    """q / k_new / v_new [B, H, D] -> fused qkv [B, 1, 3C]."""
    B, H, D = q.shape
    return torch.cat([t.reshape(B, 1, H * D) for t in (q, k_new, v_new)], dim=2).contiguous()


def _empty_cache(B, H, L_max, D):
    """An FP8 cache whose every row is the NaN byte with a NaN scale."""
    return (torch.full((B, H, L_max, D), NAN_CODE, dtype=U8, device=DEV),
            torch.full((B, H, L_max), NAN, dtype=torch.float32, device=DEV))


class _Case:
    """Random q / K / V for L keys; a NaN-filled FP8 cache holding the torch-quantised first
    L - 1 of them, the last one (bf16) as the token being decoded; length = L - 1 on the device."""

    def __init__(self, B, H, D, L, L_max, seed):
        g = torch.Generator().manual_seed(seed)
        self.q = torch.randn(B, H, D, generator=g).to(torch.bfloat16).to(DEV)
        K = torch.randn(B, H, L, D, generator=g).to(torch.bfloat16)
        V = torch.randn(B, H, L, D, generator=g).to(torch.bfloat16)
        self.kq, self.ks = _quant(K)
        self.vq, self.vs = _quant(V)
        self.kc, self.ksc = _empty_cache(B, H, L_max, D)
        self.vc, self.vsc = _empty_cache(B, H, L_max, D)
        for cache, scale, code, s in ((self.kc, self.ksc, self.kq, self.ks),
                                      (self.vc, self.vsc, self.vq, self.vs)):
            cache[:, :, :L - 1] = code[:, :, :L - 1]
            scale[:, :, :L - 1] = s[:, :, :L - 1]
        self.qkv = _pack(self.q, K[:, :, L - 1].to(DEV), V[:, :, L - 1].to(DEV))
        self.length = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
        self.H = H

    def run(self, **kw):
        return decode_attention(self.qkv, self.H, self.kc.view(E4M3), self.vc.view(E4M3),
                                self.length, k_scale=self.ksc, v_scale=self.vsc, **kw)

    def want(self, extra=0):
        """Attention over the quantised keys, the token's row ``extra`` more times."""
        Kd, Vd = _dequant(self.kq, self.ks), _dequant(self.vq, self.vs)
        Kd = torch.cat([Kd] + [Kd[:, :, -1:]] * extra, dim=2)
        Vd = torch.cat([Vd] + [Vd[:, :, -1:]] * extra, dim=2)
        return _ref(self.q, Kd, Vd)[0]

    def assert_cache(self, L, extra=0):
        """Rows < L + extra hold the quantised keys (the token ``extra`` more times), rows past
        them are untouched."""
        n = L + extra
        for cache, scale, code, s in ((self.kc, self.ksc, self.kq, self.ks),
                                      (self.vc, self.vsc, self.vq, self.vs)):
            code = torch.cat([code] + [code[:, :, -1:]] * extra, dim=2)
            s = torch.cat([s] + [s[:, :, -1:]] * extra, dim=2)
            assert torch.equal(cache[:, :, :n], code), "codes differ from _quantize_torch"
            assert torch.equal(scale[:, :, :n].view(torch.int32), s.view(torch.int32)), \
                "scales differ from _quantize_torch"
            assert (cache[:, :, n:] == NAN_CODE).all() and torch.isnan(scale[:, :, n:]).all()


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("D", [64, 128])
def test_every_key_position_is_seen_bit_exactly(D):
    """Inputs the quantiser represents losslessly: codes c (e4m3 values, one column per row forced
    to +-448) times 2^-7, so every row's scale is exactly 2^-7 and dequant(quant(k)) == k. Batch
    entry b asks for key b: q_b = 32 k_b makes key b's score lead every other by >= 30 (asserted
    from the fp32 reference), so the output must be v_b's bits — the leaked weight is < L e^-30,
    far below half a bf16 ulp. One launch, L = 2 CHUNK_FP8 + 3 keys, B = L."""
    L = 2 * CHUNK_FP8 + 3
    g = torch.Generator().manual_seed(23 + D)

    def lossless():
        c = (torch.randn(L, D, generator=g) * 96).clamp(-448, 448).to(E4M3).float()
        # a value that rounds to -0 becomes +0: a weighted sum that starts at +0 cannot return the
        # sign of a zero, so -0 has no bits to reproduce (the fp32 reference returns +0 as well)
        c[c == 0] = 0.0
        col = torch.randint(0, D, (L,), generator=g)
        sign = torch.randint(0, 2, (L,), generator=g).float() * 2 - 1
        c[torch.arange(L), col] = 448 * sign
        return (c * 2.0 ** -7).to(torch.bfloat16)

    k, v = lossless(), lossless()
    kq, ks = _quant(k)
    vq, vs = _quant(v)
    assert torch.equal(ks, torch.full_like(ks, 2.0 ** -7)) and torch.equal(ks, vs)
    k, v = k.to(DEV), v.to(DEV)
    assert torch.equal(_dequant(kq, ks), k.float()) and torch.equal(_dequant(vq, vs), v.float())
    q = (k.float() * 32).to(torch.bfloat16)                      # exact: a power of two
    assert torch.equal(q.float(), k.float() * 32)
    K = k.float()[None, None].expand(L, 1, L, D)
    V = v.float()[None, None].expand(L, 1, L, D)
    want, s = _ref(q[:, None, :], K, V)
    top2 = s[:, 0].topk(2, dim=-1)
    assert torch.equal(top2.indices[:, 0], torch.arange(L, device=DEV))
    lead = float((top2.values[:, 0] - top2.values[:, 1]).min())
    print(f"D={D} L={L}: lead {lead:.1f}")
    assert lead >= 30, lead
    assert torch.equal(_bits(want[:, 0].to(torch.bfloat16)), _bits(v))   # the reference is exact
    del K, V, want, s

    kc, ksc = _empty_cache(L, 1, L + 5, D)
    vc, vsc = _empty_cache(L, 1, L + 5, D)
    kc[:, :, :L - 1] = kq[:L - 1]
    vc[:, :, :L - 1] = vq[:L - 1]
    ksc[:, :, :L - 1] = ks[:L - 1]
    vsc[:, :, :L - 1] = vs[:L - 1]
    qkv = _pack(q[:, None, :], k[L - 1].expand(L, 1, D), v[L - 1].expand(L, 1, D))
    length = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
    got = decode_attention(qkv, 1, kc.view(E4M3), vc.view(E4M3), length, k_scale=ksc,
                           v_scale=vsc)
    torch.cuda.synchronize()
    assert got.shape == (L, 1, D)
    wrong = (_bits(got[:, 0]) != _bits(v)).any(-1).nonzero().flatten().tolist()
    assert not wrong, f"batch entries (= key positions) with a wrong output: {wrong[:20]}"
    assert torch.equal(kc[:, 0, L - 1], kq[L - 1].expand(L, D))  # the token, quantised
    assert torch.equal(ksc[:, 0, L - 1], ks[L - 1].expand(L))


LENGTHS = [(D, L) for D in (64, 128)
           for L in (1, 2, SLOTS[D] - 1, SLOTS[D], SLOTS[D] + 1, CHUNK_FP8 - 1, CHUNK_FP8,
                     CHUNK_FP8 + 1, 3 * CHUNK_FP8 + 17)]


@pytest.mark.parametrize("D,L", LENGTHS)
@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("fused", [True, False])
def test_random_inputs_match_fp32(B, H, D, L, fused):
    """Bound 2^-7 max|want|, the bf16 decode test's: the quantisation is common to both sides, so
    what remains is one bf16 rounding of the output (<= 2^-9 relative) and fp32 reassociation,
    orders below; the 4x margin is stated, not tuned. Cache rows >= L hold the NaN byte and NaN
    scales: a read past the live length would show in the output."""
    L_max = L + 37
    c = _Case(B, H, D, L, L_max, seed=1000 * D + 10 * L + B)
    got = c.run(fused=fused)
    torch.cuda.synchronize()
    want = c.want()
    got = got.view(B, H, D).float()
    assert torch.isfinite(got).all()
    ratio = float((got - want).abs().max() / want.abs().max())
    print(f"kv8 decode B={B} H={H} D={D} L={L} fused={fused}: max|got-want|/max|want| = "
          f"{ratio:.3e}")
    assert ratio <= 2.0 ** -7, f"max|got - want| / max|want| = {ratio:.3e} > 2^-7"
    c.assert_cache(L)                                             # the token at L - 1, no more
    assert int(c.length) == L - 1                                 # not advanced


@pytest.mark.parametrize("D", [64, 128])
def test_length_is_read_on_the_device(D):
    """Same host arguments twice, the device length bumped in between (across a chunk edge):
    the second call appends at the new position and attends over one key more."""
    B, H, n0 = 2, 3, CHUNK_FP8 - 1
    L_max = CHUNK_FP8 + 40
    c = _Case(B, H, D, n0 + 1, L_max, seed=77 + D)
    ws = torch.empty(dec.workspace_numel(B, H, D, L_max, CHUNK_FP8), dtype=torch.float32,
                     device=DEV)
    outs = []
    for _ in range(2):
        outs.append(c.run(len_bound=L_max, workspace=ws).view(B, H, D).float())
        c.length.add_(1)
    torch.cuda.synchronize()
    assert int(c.length) == n0 + 2
    for i, got in enumerate(outs):
        want = c.want(extra=i)
        ratio = float((got - want).abs().max() / want.abs().max())
        assert ratio <= 2.0 ** -7, (i, ratio)
    c.assert_cache(n0 + 1, extra=1)
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("at_end", [False, True])
@pytest.mark.parametrize("T", [1, 70])
@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_fp8_is_bit_exact_and_writes_nothing_else(D, T, at_end):
    """Caches and scales are contiguous views into larger sentinel-filled allocations: after the
    append every byte outside positions [length, length + T) is unchanged — inside the cache and
    in the margins on both sides — and the appended rows are ``_quantize_torch``'s bits. One row
    is all zero (scale 1, codes 0), one has a single non-zero element."""
    B, H, L_max, margin = 2, 3, 80, 4096
    rows = B * H * L_max
    start = L_max - T if at_end else 0
    g = torch.Generator().manual_seed(D + T)
    qkv = torch.randn(B, T, 3, H, D, generator=g).to(torch.bfloat16)
    qkv[0, 0, 1, 0] = 0                                          # an all-zero K row
    qkv[B - 1, T - 1, 2, H - 1] = 0
    qkv[B - 1, T - 1, 2, H - 1, D - 3] = -0.37                   # a single non-zero element in V
    qkv = qkv.view(B, T, 3 * H * D).to(DEV)
    codes = [torch.full((rows * D + 2 * margin,), s, dtype=U8, device=DEV) for s in (0x5A, 0xA5)]
    scales = [torch.full((rows + 2 * margin,), s, dtype=torch.float32, device=DEV)
              for s in (-12345.0, 54321.0)]
    kc, vc = (b[margin:margin + rows * D].view(B, H, L_max, D) for b in codes)
    ksc, vsc = (b[margin:margin + rows].view(B, H, L_max) for b in scales)
    want_c, want_s = [b.clone() for b in codes], [b.clone() for b in scales]
    for j in range(2):
        x = qkv.view(B, T, 3, H, D)[:, :, 1 + j].permute(0, 2, 1, 3)         # [B, H, T, D]
        code, s = _quant(x)
        want_c[j][margin:margin + rows * D].view(B, H, L_max, D)[:, :, start:start + T] = code
        want_s[j][margin:margin + rows].view(B, H, L_max)[:, :, start:start + T] = s
    length = torch.tensor([start], dtype=torch.int32, device=DEV)
    kv_append(qkv, H, kc.view(E4M3), vc.view(E4M3), length, pos=start, k_scale=ksc, v_scale=vsc)
    torch.cuda.synchronize()
    for b, w in zip(codes, want_c):
        assert torch.equal(b, w)
    for b, w in zip(scales, want_s):
        assert torch.equal(b.view(torch.int32), w.view(torch.int32))
    assert float(ksc[0, 0, start]) == 1.0 and not kc[0, 0, start].any()
    assert int((vc[B - 1, H - 1, start + T - 1] != 0).sum()) == 1
    with pytest.raises(ValueError):                                          # host overflow check
        kv_append(qkv, H, kc.view(E4M3), vc.view(E4M3), length, pos=L_max - T + 1, k_scale=ksc,
                  v_scale=vsc)


def test_two_runs_are_bit_identical():
    B, H, D, L = 2, 3, 128, 3 * CHUNK_FP8 + 17
    outs = []
    for _ in range(2):
        outs.append(_Case(B, H, D, L, L + 37, seed=9).run())
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize("D", [64, 128])
def test_graph_replay_walks_the_positions(D):
    """One captured decode_attention + length.add_(1), replayed 5 times on fixed inputs (single
    stream, no forked branches): after every replay the output equals the eager result for that
    position bit-exactly and the cache's newest row is the quantised token."""
    B, H, p, steps = 2, 3, CHUNK_FP8 - 2, 5
    L_max = p + steps + 3
    c = _Case(B, H, D, p + 1, L_max, seed=31 + D)
    ws = torch.empty(dec.workspace_numel(B, H, D, L_max, CHUNK_FP8), dtype=torch.float32,
                     device=DEV)
    kc2, vc2, ksc2, vsc2 = c.kc.clone(), c.vc.clone(), c.ksc.clone(), c.vsc.clone()
    len2 = c.length.clone()

    def step2():
        return decode_attention(c.qkv, H, kc2.view(E4M3), vc2.view(E4M3), len2, len_bound=L_max,
                                workspace=ws, k_scale=ksc2, v_scale=vsc2)

    eager = []
    for _ in range(steps):
        eager.append(c.run(len_bound=L_max, workspace=ws).clone())
        c.length.add_(1)
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up: writes row p, the same token
        step2()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step2()
        len2.add_(1)
    assert int(len2) == p                                # the capture ran nothing
    for i in range(steps):
        graph.replay()
        torch.cuda.synchronize()
        assert int(len2) == p + i + 1
        assert torch.equal(_bits(out), _bits(eager[i])), f"replay {i}"
        assert torch.equal(kc2[:, :, p + i], c.kq[:, :, -1])
        assert torch.equal(vc2[:, :, p + i], c.vq[:, :, -1])
        assert torch.equal(ksc2[:, :, p + i], c.ks[:, :, -1])
        assert torch.equal(vsc2[:, :, p + i], c.vs[:, :, -1])
    assert (kc2[:, :, p + steps:] == NAN_CODE).all() and torch.isnan(ksc2[:, :, p + steps:]).all()
    assert not torch.equal(_bits(eager[0]), _bits(eager[-1]))


KW = dict(hidden_size=256, num_layers=2, ffn_intermediate=1024, seed=11, init_std=0.05)


def _decode_rows(model, x, prompt):
    cache = model.new_kv_cache(x.shape[0], x.shape[1])
    rows = [model(x[:, :prompt].contiguous(), kv_cache=cache)]
    for t in range(prompt, x.shape[1]):
        rows.append(model(x[:, t:t + 1].contiguous(), kv_cache=cache))
    assert cache.pos == x.shape[1] and int(cache.length) == x.shape[1]
    return torch.cat(rows, dim=1).float(), cache


@pytest.mark.parametrize("heads,w8", [(4, False), (2, False), (2, True)])
def test_model_decode_with_the_fp8_cache(heads, w8):
    """Head dim 64 (4 heads) and 128 (2 heads): 48 prompt tokens + 16 decode steps on ``flash``
    with the FP8 cache against the same model in torch (``kernels="torch"``, sdpa, the same
    knobs). Bound 3e-2 of max|ref| (the project's TP-vs-dense bound). Every step of every layer
    runs the FP8 kernel; the distance to the bf16-cache decode is printed and is not zero."""
    from distributed_llm_backend_benchmark_amd import ops as O
    from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
    from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

    dev = torch.device("cuda", 0)
    knobs = dict(num_heads=heads, decode_weight_dtype="fp8" if w8 else "bf16", **KW)
    model = LLM(comm=Comm(0, 1, 0, "gloo", dev), attention="flash", kv_cache_dtype="fp8", **knobs)
    torch_model = LLM(comm=Comm(0, 1, 0, "gloo", dev), attention="sdpa", kernels="torch",
                      kv_cache_dtype="fp8", **knobs)
    torch_model.load_state_dict(model.state_dict())
    plain = LLM(comm=Comm(0, 1, 0, "gloo", dev), attention="flash", **knobs)
    plain.load_state_dict(model.state_dict())
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(2, 64, 256, generator=g, device=dev).to(torch.bfloat16)
    ref, _ = _decode_rows(torch_model, x, 48)
    calls = [0, 0]
    real = O.decode_attention

    def counted(qkv, n_head, k_cache, v_cache, length, **kw):
        ks, vs = kw.get("k_scale"), kw.get("v_scale")
        calls[0] += 1
        calls[1] += int(ks is not None and k_cache.dtype == E4M3 and dec.use_hip(qkv)
                        and dec.hip_supported(qkv, n_head, k_cache, v_cache, ks, vs))
        return real(qkv, n_head, k_cache, v_cache, length, **kw)

    O.decode_attention = counted
    try:
        got, cache = _decode_rows(model, x, 48)
    finally:
        O.decode_attention = real
    base, _ = _decode_rows(plain, x, 48)
    torch.cuda.synchronize()
    assert calls == [16 * 2, 16 * 2], calls            # every step of every layer, on the kernel
    assert cache.kv_dtype == "fp8" and cache.k[0].dtype == E4M3
    err = float((got - ref).abs().max() / ref.abs().max())
    dist = float((got - base).abs().max() / base.abs().max())
    print(f"kv8 decode vs torch, heads={heads} w8={w8}: {err:.3e}; vs the bf16-cache decode: "
          f"{dist:.3e}")
    assert err < 3e-2, err
    assert dist > 0


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


def _run_tp(cfg_path, *extra):
    return subprocess.run([sys.executable, "-m", "distributed_llm_backend_benchmark_amd.cli.run_tp",
                           "--config", str(cfg_path), "--backend", "rccl", *extra],
                          capture_output=True, text=True, timeout=600, cwd=REPO)


def test_run_tp_decode_kv_cache_fp8(tmp_path):
    p, name = _cfg(tmp_path)
    out = _run_tp(p, "--decode", "8", "--attention", "flash", "--kv-cache", "fp8")
    assert out.returncode == 0, out.stderr[-3000:]
    files = [f for f in os.listdir(tmp_path) if f.endswith(".json")]
    assert files == [f"rccl_{name}_decode8_kv8.json"], files
    d = json.load(open(tmp_path / files[0]))["decode"]
    assert d["timing_mode"] == "hip_graph_replay", d["hip_graph_note"]
    assert d["attention_path"] == "hip" and d["kv_dtype"] == "fp8"
    assert d["kv_cache_bytes_per_rank"] == 2 * 2 * 2 * 8 * 72 * (64 + 4) == 313344
    assert d["kv_bytes_read_per_step_mean"] == (64 + 4.5) * 2 * 2 * 8 * 2 * (64 + 4)
    assert len(d["ms_per_token"]) == 3 and all(v > 0 for v in d["ms_per_token"])


@pytest.mark.parametrize("extra", [["--attention", "flash"],
                                   ["--decode", "8", "--attention", "slice"]])
def test_run_tp_kv_cache_fp8_refusals(tmp_path, extra):
    """No decode tokens, or the stateless slice stub: exit code 1, ERROR, no JSON."""
    p, _ = _cfg(tmp_path)
    out = _run_tp(p, "--kv-cache", "fp8", *extra)
    assert out.returncode == 1 and "ERROR" in out.stdout, out.stderr[-3000:]
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".json")]
