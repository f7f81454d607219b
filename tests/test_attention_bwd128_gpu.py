"""Causal attention backward at head dim 128 (csrc/attention.hip, attn_bwd_dq_d128_kernel and
attn_bwd_dkdv_d128_kernel) against the fp32 autograd reference: odd lengths, the two image
halves of a 128-wide head, determinism, the timeline stamps and the autograd path.

Bound (the project's own for head dim 64): max|got - want| <= 0.03 max|want| + 0.02 for each of
dQ, dK and dV."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128


def _ref(qkv, H):
    B, T, C3 = qkv.shape
    C = C3 // 3
    d = C // H
    q, k, v = qkv.float().view(B, T, 3, H, d).permute(2, 0, 3, 1, 4).unbind(0)
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    mask = torch.ones(T, T, device=qkv.device, dtype=torch.bool).triu(1)
    s = s.masked_fill(mask, float("-inf"))
    lse = torch.logsumexp(s, -1)
    o = torch.softmax(s, -1) @ v
    return o.transpose(1, 2).reshape(B, T, C), lse


def _ref_grads(qkv, gout, H):
    x = qkv.float().clone().requires_grad_(True)
    y, _ = _ref(x, H)
    y.backward(gout.float())
    return y.detach(), x.grad


def _inputs(B, T, H, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    qkv = (torch.randn(B, T, 3 * H * D, device="cuda", generator=g) * scale).to(torch.bfloat16)
    gout = (torch.randn(B, T, H * D, device="cuda", generator=g) * scale).to(torch.bfloat16)
    return qkv, gout


def _errors(d, ref, H):
    """[(name, max abs error, max |want|)] for dQ, dK, dV of a fused [B, T, 3C] gradient."""
    C = H * D
    out = []
    for j, name in enumerate(("dq", "dk", "dv")):
        got, want = d[..., j * C:(j + 1) * C].float(), ref[..., j * C:(j + 1) * C]
        out.append((name, float((got - want).abs().max()), float(want.abs().max())))
    return out


def _within(errs):
    return all(err <= 0.03 * scale + 0.02 for _, err, scale in errs)


@pytest.mark.parametrize("B,T,H", [(1, 17, 1), (1, 64, 1), (2, 200, 3), (1, 256, 2), (1, 333, 2),
                                   (2, 1024, 2)])
def test_attn_bwd128_matches_fp32_reference(B, T, H):
    """Less than one wave of rows, T not a tile multiple with an odd head count, one paired
    workgroup, a single-pass middle block, and every pairing of eight blocks. The library
    backward's error on the same inputs rides in the message: ours failing a bound that it passes
    is a kernel bug."""
    from distributed_llm_backend_benchmark_amd.ops.attention import (attn_bwd, attn_bwd_library,
                                                                     attn_fwd)

    qkv, gout = _inputs(B, T, H, 7 * T + H)
    out, lse = attn_fwd(qkv, H)
    d = attn_bwd(qkv, out, lse, gout, H)
    _, ref = _ref_grads(qkv, gout, H)
    ours = _errors(d, ref, H)
    lib = _errors(attn_bwd_library(qkv, out, lse, gout, H), ref, H)
    print("ours", ours, "library", lib)
    assert bool(torch.isfinite(d.float()).all())
    assert _within(ours), {"ours": ours, "library": lib}


@pytest.mark.parametrize("live", [0, 1])
def test_attn_bwd128_column_halves(live):
    """Q, K, V and dO zero in one 64-dim half of every head: the gradients are exactly zero there
    and within the bound in the other half (a swapped or mixed image half or accumulator block
    would leak)."""
    from distributed_llm_backend_benchmark_amd.ops.attention import attn_bwd, attn_fwd

    B, T, H = 1, 333, 2
    qkv, gout = _inputs(B, T, H, 11 + live)
    dead = slice(64 * (1 - live), 64 * (2 - live))
    q5 = qkv.view(B, T, 3, H, D)
    q5[..., dead] = 0
    gout.view(B, T, H, D)[..., dead] = 0
    out, lse = attn_fwd(qkv, H)
    d = attn_bwd(qkv, out, lse, gout, H)
    assert bool((d.view(B, T, 3, H, D)[..., dead] == 0).all())
    _, ref = _ref_grads(qkv, gout, H)
    errs = _errors(d, ref, H)
    print(errs)
    assert _within(errs), errs


def test_attn_bwd128_scaled_scores():
    from distributed_llm_backend_benchmark_amd.ops.attention import attn_bwd, attn_fwd

    B, T, H = 2, 512, 2
    qkv, gout = _inputs(B, T, H, 5, scale=1.5)
    out, lse = attn_fwd(qkv, H)
    d = attn_bwd(qkv, out, lse, gout, H)
    assert bool(torch.isfinite(d.float()).all())
    _, ref = _ref_grads(qkv, gout, H)
    errs = _errors(d, ref, H)
    print(errs)
    assert _within(errs), errs


def test_attn_bwd128_deterministic_and_stamped():
    """No atomics: two calls are bit-identical, also with the timeline stamps on, and then every
    workgroup of the dQ and dK/dV kernels records start <= mid <= end."""
    from distributed_llm_backend_benchmark_amd.ops import _lib
    from distributed_llm_backend_benchmark_amd.ops.attention import attn_bwd, attn_fwd

    B, T, H = 2, 1024, 4
    qkv, gout = _inputs(B, T, H, 3)
    out, lse = attn_fwd(qkv, H)
    d0 = attn_bwd(qkv, out, lse, gout, H)
    d1 = attn_bwd(qkv, out, lse, gout, H)
    assert torch.equal(d0, d1)
    nwg = ((T + 127) // 128 + 1) // 2 * H * B      # both kernels: 128-row blocks, paired
    st = [torch.zeros(nwg, 4, dtype=torch.int64, device="cuda") for _ in range(3)]
    L = _lib.lib()
    L.dlbb_attn_set_stamps(st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr())
    try:
        d2 = attn_bwd(qkv, out, lse, gout, H)
        torch.cuda.synchronize()
    finally:
        L.dlbb_attn_set_stamps(None, None, None)
    assert torch.equal(d0, d2)
    assert not bool(st[0].any())                   # no forward ran
    for t in st[1:]:
        a = t.cpu()
        assert bool((a[:, 0] > 0).all()) and bool((a[:, 2] >= a[:, 0]).all())
        assert bool(((a[:, 1] >= a[:, 0]) & (a[:, 1] <= a[:, 2])).all())   # nkb = 8: all paired


def test_causal_attention_autograd_d128_needs_no_library(monkeypatch):
    from distributed_llm_backend_benchmark_amd.ops import attention, causal_attention

    def boom(*a, **k):
        raise AssertionError("library attention backward called on the autograd path")

    monkeypatch.setattr(attention, "attn_bwd_library", boom)
    B, T, H = 2, 512, 4
    base, gout = _inputs(B, T, H, 3)
    x1 = base.clone().requires_grad_(True)
    causal_attention(x1, H).backward(gout)
    x2 = base.clone().requires_grad_(True)
    attention._torch_attention(x2, H).backward(gout)
    torch.testing.assert_close(x1.grad.float(), x2.grad.float(), rtol=3e-2, atol=3e-2)


def test_attn_bwd128_noncontiguous_dout():
    from distributed_llm_backend_benchmark_amd.ops.attention import attn_bwd, attn_fwd

    B, T, H = 1, 200, 2
    qkv, _ = _inputs(B, T, H, 9)
    g = torch.Generator(device="cuda").manual_seed(10)
    gout = torch.randn(B, H * D, T, device="cuda", generator=g).to(torch.bfloat16).transpose(1, 2)
    assert not gout.is_contiguous()
    out, lse = attn_fwd(qkv, H)
    assert torch.equal(attn_bwd(qkv, out, lse, gout, H),
                       attn_bwd(qkv, out, lse, gout.contiguous(), H))
