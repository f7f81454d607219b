"""The MXFP4 (e2m1 + e8m0) KV-cache kernels (csrc/attn_decode.hip) against an fp32 softmax over the
DEQUANTISED torch-quantised K / V (``ops.mxfp4._quantize_rows``), so both sides see the same codes
and scale bytes; bit-exact quantising appends, every key position, ragged rows, HIP-graph replay,
the model's decode with ``kv_cache_dtype="mxfp4"`` and the ``run_tp --kv-cache mxfp4`` record."""

import json
import os

import pytest
import torch

from distributed_llm_backend_benchmark_amd.ops import decode as dec
from distributed_llm_backend_benchmark_amd.ops.decode import (CHUNK_MXFP4, decode_attention,
                                                              kv_append)
from distributed_llm_backend_benchmark_amd.ops.mxfp4 import _quantize_rows
from test_decode_kv8_gpu import KW, _bits, _cfg, _decode_rows, _pack, _ref, _run_tp

pytestmark = pytest.mark.gpu

DEV = "cuda"
CODE, SCALE = 0x77, 0xFF             # dead rows: codes 6 | 6 under the scale byte "NaN" (inf as a float)
SLOTS = {64: 64, 128: 32}            # key slots per workgroup: 256 threads / (D / 16 lanes per key)
CH = CHUNK_MXFP4


def _quant(x):
    """``_quantize_rows`` of CPU rows [..., D] -> (codes [..., D/2], scale bytes [..., D/32]), on
    the device."""
    D = x.shape[-1]
    code, scale = _quantize_rows(x.cpu().float().reshape(-1, D))
    return (code.view(*x.shape[:-1], D // 2).to(DEV), scale.view(*x.shape[:-1], D // 32).to(DEV))


def _dead(B, H, L_max, D):
    return (torch.full((B, H, L_max, D // 2), CODE, dtype=torch.uint8, device=DEV),
            torch.full((B, H, L_max, D // 32), SCALE, dtype=torch.uint8, device=DEV))


class _Case:
    """Random q / K / V for L keys; a dead-filled MXFP4 cache holding the torch-quantised first
    L - 1 of them, the last one (bf16) as the token being decoded; length = L - 1 on the device."""

    def __init__(self, B, H, D, L, L_max, seed):
        g = torch.Generator().manual_seed(seed)
        self.q = torch.randn(B, H, D, generator=g).to(torch.bfloat16).to(DEV)
        K, V = (torch.randn(B, H, L, D, generator=g).to(torch.bfloat16) for _ in range(2))
        self.quant = [_quant(K), _quant(V)]                       # (codes, scales) of K, of V
        self.cache = [_dead(B, H, L_max, D), _dead(B, H, L_max, D)]
        for (cc, sc), (code, s) in zip(self.cache, self.quant):
            cc[:, :, :L - 1], sc[:, :, :L - 1] = code[:, :, :L - 1], s[:, :, :L - 1]
        self.qkv = _pack(self.q, K[:, :, L - 1].to(DEV), V[:, :, L - 1].to(DEV))
        self.length = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
        self.H = H

    def run(self, **kw):
        (kc, ks), (vc, vs) = self.cache
        return decode_attention(self.qkv, self.H, kc, vc, self.length, k_scale=ks, v_scale=vs, **kw)

    def want(self):
        return _ref(self.q, *(dec.dequantize(code, s) for code, s in self.quant))[0]

    def assert_cache(self, L):
        """Rows < L hold ``_quantize_rows``' bits (the token at L - 1), rows past them are dead."""
        for (cc, sc), (code, s) in zip(self.cache, self.quant):
            assert torch.equal(cc[:, :, :L], code) and torch.equal(sc[:, :, :L], s)
            assert (cc[:, :, L:] == CODE).all() and (sc[:, :, L:] == SCALE).all()


@pytest.mark.parametrize("seq", [False, True])
@pytest.mark.parametrize("at_end", [False, True])
@pytest.mark.parametrize("T", [1, 70])
@pytest.mark.parametrize("D", [64, 128])
def test_kv_append_mxfp4_is_bit_exact_and_writes_nothing_else(D, T, at_end, seq):
    """Caches and scales are views into larger sentinel-filled allocations: after the append every
    byte outside the appended rows is unchanged and those rows are ``_quantize_rows``' bits. The
    first K block holds 7.5 (scale byte 127, in (6, 8): saturates), the ties 0.25 0.75 1.25 2.5 3.5
    5 and negatives that round to -0; another block is all zero. Per sequence: row 1 is an empty
    slot and the last tokens of row 2 fall past L_max."""
    B, H, L_max, margin = 3, 3, 80, 4096
    rows = B * H * L_max
    start = L_max - T if at_end else 0
    lens = [start, -1, L_max - T + (2 if T > 1 else 0)] if seq else [start] * B
    g = torch.Generator().manual_seed(D + T)
    qkv = torch.randn(B, T, 3, H, D, generator=g).to(torch.bfloat16)
    qkv[0, 0, 1, 0, :32] = 0
    qkv[0, 0, 1, 0, :9] = torch.tensor([7.5, 0.25, 0.75, 1.25, 2.5, 3.5, 5, -0.25, -0.1])
    qkv[B - 1, 0, 2, H - 1, 32:64] = 0                           # an all-zero block of V
    want, got = [], []
    for j in range(2):
        cw = torch.full((rows * (D // 2) + 2 * margin,), 0x5A + j, dtype=torch.uint8)
        sw = torch.full((rows * (D // 32) + 2 * margin,), 0xA5 + j, dtype=torch.uint8)
        got += [cw.to(DEV), sw.to(DEV)]
        code, s = _quantize_rows(qkv[:, :, 1 + j].float().reshape(-1, D))
        code, s = code.view(B, T, H, D // 2), s.view(B, T, H, D // 32)
        for b, n in enumerate(lens):
            keep = max(0, min(T, L_max - n)) if n >= 0 else 0
            for w, x in ((cw, code), (sw, s)):
                view = w[margin:-margin].view(B, H, L_max, -1)
                view[b, :, n:n + keep] = x[b, :keep].transpose(0, 1)
        want += [cw, sw]
    kc, ksc, vc, vsc = (t[margin:-margin].view(B, H, L_max, -1) for t in got)
    length = torch.tensor(lens if seq else [start], dtype=torch.int32, device=DEV)
    kv_append(qkv.view(B, T, 3 * H * D).to(DEV), H, kc, vc, length, k_scale=ksc, v_scale=vsc)
    torch.cuda.synchronize()
    for a, w in zip(got, want):
        assert torch.equal(a.cpu(), w)
    assert int(ksc[0, 0, start, 0]) == 127 and kc[0, 0, start, :5].tolist() == \
        [0x07, 0x22, 0x64, 0x86, 0x08]                           # 6 0 | 1 1 | 2 4 | 4 -0 | -0 0
    if not seq:
        with pytest.raises(ValueError):                          # host overflow check
            kv_append(qkv.view(B, T, -1).to(DEV), H, kc, vc, length, pos=L_max - T + 1,
                      k_scale=ksc, v_scale=vsc)


@pytest.mark.parametrize("D,L", [(D, L) for D in (64, 128) for L in (
    1, 2, SLOTS[D] - 1, SLOTS[D], SLOTS[D] + 1, CH - 1, CH, CH + 1, 3 * CH + 17)])
@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("fused", [True, False])
def test_random_inputs_match_fp32(B, H, D, L, fused):
    """Bound 2^-7 max|want|, the bf16 and FP8 decode tests': the quantisation is common to both
    sides, what remains is one bf16 rounding of the output (<= 2^-9 relative) and fp32
    reassociation, orders below. Cache rows >= L hold codes 0x77 under scale byte 0xFF (inf): a
    read past the live length would show as inf / NaN."""
    c = _Case(B, H, D, L, L + 37, seed=1000 * D + 10 * L + B)
    got = c.run(fused=fused).view(B, H, D).float()
    torch.cuda.synchronize()
    want = c.want()
    assert torch.isfinite(got).all()
    ratio = float((got - want).abs().max() / want.abs().max())
    print(f"kv4 decode B={B} H={H} D={D} L={L} fused={fused}: {ratio:.3e}")
    assert ratio <= 2.0 ** -7, f"max|got - want| / max|want| = {ratio:.3e} > 2^-7"
    c.assert_cache(L)                                             # the token at L - 1, no more
    assert int(c.length) == L - 1                                 # not advanced


@pytest.mark.parametrize("D", [64, 128])
def test_every_key_position_is_seen_bit_exactly(D):
    """Lossless inputs: e2m1 grid values times 2^-3 with one column per 32-block forced to +-6, so
    every scale byte is 124 and dequant(quant(x)) == x; -0 is normalised to +0. Batch entry b asks
    for key b with q_b = 512 k_b: its score leads every other by >= 30 (asserted from the fp32
    reference on the CPU; here by > 104, so every other weight underflows to 0 and a zero element
    of v_b comes back as 0), so the output must be v_b's bits. L = 2 CHUNK_MXFP4 + 3 = B."""
    L = 2 * CH + 3
    g = torch.Generator().manual_seed(23 + D)
    grid = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6])

    def lossless():
        x = grid[torch.randint(0, 8, (L, D), generator=g)]
        x = x * (torch.randint(0, 2, (L, D), generator=g) * 2 - 1) + 0.0     # -0 -> +0
        col = torch.randint(0, 32, (L, D // 32), generator=g) + torch.arange(0, D, 32)
        x.scatter_(1, col, 6.0 * (torch.randint(0, 2, col.shape, generator=g) * 2 - 1))
        return (x * 2.0 ** -3).to(torch.bfloat16)

    k, v = lossless(), lossless()
    (kq, ks), (vq, vs) = _quant(k), _quant(v)
    assert (ks == 124).all() and (vs == 124).all()
    assert torch.equal(dec.dequantize(kq, ks).cpu(), k.float())
    assert torch.equal(dec.dequantize(vq, vs).cpu(), v.float())
    q = (k.float() * 512).to(torch.bfloat16)
    s = q.float() @ k.float().T / D ** 0.5                       # entry b over the L keys
    top2 = s.topk(2, dim=-1)
    assert torch.equal(top2.indices[:, 0], torch.arange(L))
    lead = float((top2.values[:, 0] - top2.values[:, 1]).min())
    assert lead >= 30, lead
    want = torch.softmax(s, -1) @ v.float()
    assert torch.equal(_bits(want.to(torch.bfloat16)), _bits(v))  # the reference is exact
    (kc, ksc), (vc, vsc) = _dead(L, 1, L + 5, D), _dead(L, 1, L + 5, D)
    kc[:, 0, :L - 1], ksc[:, 0, :L - 1] = kq[:L - 1], ks[:L - 1]
    vc[:, 0, :L - 1], vsc[:, 0, :L - 1] = vq[:L - 1], vs[:L - 1]
    qkv = _pack(q[:, None, :], k[L - 1].expand(L, 1, D), v[L - 1].expand(L, 1, D)).to(DEV)
    length = torch.tensor([L - 1], dtype=torch.int32, device=DEV)
    got = decode_attention(qkv, 1, kc, vc, length, k_scale=ksc, v_scale=vsc)
    torch.cuda.synchronize()
    wrong = (_bits(got[:, 0]) != _bits(v.to(DEV))).any(-1).nonzero().flatten().tolist()
    assert not wrong, f"batch entries (= key positions) with a wrong output: {wrong[:20]}"
    assert torch.equal(kc[:, 0, L - 1], kq[L - 1].expand(L, D // 2))         # the token, quantised
    assert (ksc[:, 0, L - 1] == 124).all()


@pytest.mark.parametrize("D", [64, 128])
def test_ragged_rows_have_the_bits_of_batch_one_launches(D):
    """Lengths 0, a chunk edge, a long row, an empty slot, a chunk edge less one: row b of the
    per-sequence launch has the bits of a batch-1 shared-length launch at length[b]; the empty
    slot's row is zeros and its cache untouched."""
    H, lens = 3, [0, CH, 2 * CH + 70, -1, CH - 1]
    B, L_max = len(lens), 2 * CH + 80
    c = _Case(B, H, D, L_max, L_max, seed=57 + D)                 # a full random cache
    (kc, ks), (vc, vs) = c.cache
    kc[:, :, -1], vc[:, :, -1] = c.quant[0][0][:, :, -1], c.quant[1][0][:, :, -1]
    ks[:, :, -1], vs[:, :, -1] = c.quant[0][1][:, :, -1], c.quant[1][1][:, :, -1]
    for b, n in enumerate(lens):                                  # rows past each length: dead
        for t, fill in ((kc, CODE), (vc, CODE), (ks, SCALE), (vs, SCALE)):
            t[b, :, max(n, 0):] = fill
    ones = [[t[b:b + 1].clone() for t in (kc, vc, ks, vs)] for b in range(B)]
    length = torch.tensor(lens, dtype=torch.int32, device=DEV)
    got = decode_attention(c.qkv, H, kc, vc, length, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        if n < 0:
            assert not got[b].any() and (kc[b] == CODE).all() and (ks[b] == SCALE).all()
            continue
        k1, v1, ks1, vs1 = ones[b]
        one = decode_attention(c.qkv[b:b + 1], H, k1, v1, length[b:b + 1].clone(), k_scale=ks1,
                               v_scale=vs1)
        assert torch.equal(_bits(got[b:b + 1]), _bits(one)), f"row {b}"
        assert torch.equal(kc[b:b + 1], k1) and torch.equal(vs[b:b + 1], vs1)


@pytest.mark.parametrize("D", [64, 128])
def test_graph_replay_walks_the_positions(D):
    """One captured decode_attention + length.add_(1), replayed 5 times across a chunk edge: every
    replay gives the eager step's bits, in the output and in the appended codes and scales."""
    B, H, p, steps = 2, 3, CH - 2, 5
    L_max = p + steps + 3
    c = _Case(B, H, D, p + 1, L_max, seed=31 + D)
    ws = torch.empty(dec.workspace_numel(B, H, D, L_max, CH), dtype=torch.float32, device=DEV)
    (kc2, ks2), (vc2, vs2) = [[t.clone() for t in pair] for pair in c.cache]
    len2 = c.length.clone()

    def step2():
        return decode_attention(c.qkv, H, kc2, vc2, len2, len_bound=L_max, workspace=ws,
                                k_scale=ks2, v_scale=vs2)

    eager = []
    for _ in range(steps):
        eager.append(c.run(len_bound=L_max, workspace=ws).clone())
        c.length.add_(1)
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
    for i in range(steps):
        graph.replay()
        torch.cuda.synchronize()
        assert int(len2) == p + i + 1
        assert torch.equal(_bits(out), _bits(eager[i])), f"replay {i}"
    (kc, ks), (vc, vs) = c.cache
    for a, e in ((kc2, kc), (ks2, ks), (vc2, vc), (vs2, vs)):
        assert torch.equal(a, e)
    assert torch.equal(kc2[:, :, p + steps - 1], c.quant[0][0][:, :, -1])
    assert (kc2[:, :, p + steps:] == CODE).all() and (ks2[:, :, p + steps:] == SCALE).all()
    assert not torch.equal(_bits(eager[0]), _bits(eager[-1]))


@pytest.mark.parametrize("heads", [4, 2])
def test_model_decode_with_the_mxfp4_cache(heads):
    """Head dim 64 (4 heads) and 128 (2 heads): 48 prompt tokens + 16 decode steps on ``flash``
    with the MXFP4 cache against the same model's torch forms (``kernels="torch"``, sdpa). The
    activations are computed separately on the two sides, so a code can flip. Measured on the
    MI355X: 1.163e-2 (4 heads) and 1.172e-2 (2 heads) of max|ref|; the bound is 2.5 x the larger,
    2.93e-2."""
    from distributed_llm_backend_benchmark_amd.models.tp_transformer import LLM
    from distributed_llm_backend_benchmark_amd.parallel.comm import Comm

    dev = torch.device("cuda", 0)
    knobs = dict(num_heads=heads, kv_cache_dtype="mxfp4", **KW)
    model = LLM(comm=Comm(0, 1, 0, "gloo", dev), attention="flash", **knobs)
    torch_model = LLM(comm=Comm(0, 1, 0, "gloo", dev), attention="sdpa", kernels="torch", **knobs)
    torch_model.load_state_dict(model.state_dict())
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(2, 64, 256, generator=g, device=dev).to(torch.bfloat16)
    ref, _ = _decode_rows(torch_model, x, 48)
    got, cache = _decode_rows(model, x, 48)
    assert cache.kv_dtype == "mxfp4" and cache.k[0].dtype == torch.uint8
    assert tuple(cache.k_scale[0].shape) == (2, heads, 64, 256 // heads // 32)
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"kv4 decode vs torch, heads={heads}: {err:.3e}")
    assert err < 2.93e-2, err


def test_run_tp_decode_kv_cache_mxfp4(tmp_path):
    p, name = _cfg(tmp_path)
    out = _run_tp(p, "--decode", "8", "--attention", "flash", "--kv-cache", "mxfp4")
    assert out.returncode == 0, out.stderr[-3000:]
    files = [f for f in os.listdir(tmp_path) if f.endswith(".json")]
    assert files == [f"rccl_{name}_decode8_kv4.json"], files
    d = json.load(open(tmp_path / files[0]))["decode"]
    assert d["timing_mode"] == "hip_graph_replay", d["hip_graph_note"]
    assert d["attention_path"] == "hip" and d["kv_dtype"] == "mxfp4"
    assert d["kv_cache_bytes_per_rank"] == 2 * 2 * 2 * 8 * 72 * (32 + 2) == 156672
    assert d["kv_bytes_read_per_step_mean"] == (64 + 4.5) * 2 * 2 * 8 * 2 * (32 + 2)
