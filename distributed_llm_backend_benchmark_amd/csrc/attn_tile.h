// Tile geometry, LDS swizzles and lane helpers shared by the MFMA attention kernels that sweep
// 8-KiB K / V images with 4 waves x 32 queries (attention.hip's causal forward, attn_prefill.hip).
#pragma once

#include "common.h"

namespace dlbb {

constexpr int kQB = 128;        // queries per workgroup
constexpr int kAttnThreads = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// 16-B chunk c (0..7) of LDS row r is stored in slot c ^ swz(r)
__device__ __forceinline__ int kswz(int r) { return (r >> 1) & 7; }
__device__ __forceinline__ int vswz(int r) { return ((r >> 1) & 1) << 2; }

__device__ __forceinline__ void attn_glds16(const void* g, char* lds) {
  __builtin_amdgcn_global_load_lds(g, (lds_vptr_t)(lds), 16, 0, 0);
}

// Block -> (block-in-head, h, b) for a (blocks-per-head, H, B) grid. xcd = 1: XCD-aware
// bijective remap (guide T1; blockIdx % 8 labels the blocks that share an L2) so each XCD's
// eighth of the grid is a contiguous run of WHOLE heads — a head's K/V (forward, dQ) or Q/dO
// (dK/dV) tiles are then fetched into one L2 instead of into all eight (the default dispatch
// sends the consecutive blocks of one head to eight different XCDs). Order inside a head kept.
__device__ __forceinline__ void head_block(int xcd_on, int& blk, int& h, int& b) {
  const int nb = gridDim.x, H = gridDim.y;
  if (!xcd_on) {
    blk = blockIdx.x;
    h = blockIdx.y;
    b = blockIdx.z;
    return;
  }
  const int nwg = nb * H * gridDim.z;
  const int L = blockIdx.x + nb * (blockIdx.y + H * blockIdx.z);
  const int x = L % 8, q = nwg / 8, r = nwg % 8;
  const int wid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + L / 8;
  blk = wid % nb;
  const int hh = wid / nb;
  h = hh % H;
  b = hh / H;
}

// lane ^ 32 half exchange of a per-lane value by v_permlane32_swap (a VALU op) instead of a
// ds_bpermute LDS round trip; max over both halves ends in every lane
__device__ __forceinline__ float xhalf_max(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false,
                                                  false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

// Forward tile geometry per head dim: one 8-KiB image per K / V tile — 64 keys x 128 B at
// D = 64, 32 keys x 256 B at D = 128 (the TP model's heads, models/tp_transformer.py) — so both
// keep 32 KiB of LDS per workgroup (double-buffered K and V) and 2 DMA wave-instructions per
// wave per image.
template <int D>
struct FwdGeo {
  static constexpr int KB = 8192 / (2 * D);   // keys per tile
  static constexpr int NKK = KB / 32;         // 32-key halves per tile
  static constexpr int NKS = D / 16;          // k-steps of S^T = K Q^T
  static constexpr int NDT = D / 32;          // 32-dim blocks of O^T
  static constexpr int ROW = 2 * D;           // image row bytes
  static constexpr int RPI = 1024 / ROW;      // rows per DMA wave-instruction
  static constexpr int TILE = KB * ROW;       // 8 KiB
};
// K image (ds_read_b128 row reads) and V image (ds_read_b64_tr_b16) swizzles: 16-B chunk c of
// row r in slot c ^ swz(r). D = 64 (128-B rows): kswz / vswz above. D = 128 (256-B rows: every
// row covers all 64 banks): r & 15 makes the 16 rows of each ds_read_b128 lane group hit 16
// distinct bank quads; (r & 3) << 2 puts the 4 rows of a transposed read's 32-lane group in 4
// distinct 64-B bank segments.
template <int D>
__device__ __forceinline__ int kswz_d(int r) { return D == 64 ? kswz(r) : (r & 15); }
template <int D>
__device__ __forceinline__ int vswz_d(int r) { return D == 64 ? vswz(r) : ((r & 3) << 2); }

// Rotary position embedding of the grouped-query kernels (attn_decode_gqa.hip, attn_prefill_gqa*),
// rotate-half (NeoX / HF Llama) pairing: column i < D / 2 of a Q or K row is paired with column
// i + D / 2. The angles come from a table: row p of `rope` (fp32 [P, D], 16-byte aligned) holds
// cos in [0, D / 2) and sin in [D / 2, D) for cache position p, so every scaling scheme is the
// table builder's business and the kernels compute no trigonometry. rope_rotate8 rotates 8
// columns c .. c + 7 of the low half (`lo`) with their partners (`hi`); `cs` points at the row's
// cos of column c (c a multiple of 8), its sin is `half` = D / 2 floats further:
//   lo' = lo cos - hi sin, hi' = hi cos + lo sin, in fp32, each rounded to bf16 once.
// V is u16x8 (a cache row on its way through the append) or bf16x8 (a Q fragment held for the
// MFMAs). With cos = 1, sin = 0 every finite value comes back with its bits.
template <typename V>
__device__ __forceinline__ void rope_rotate8(V& lo, V& hi, const float* cs, int half) {
  const f32x4 c0 = *reinterpret_cast<const f32x4*>(cs);
  const f32x4 c1 = *reinterpret_cast<const f32x4*>(cs + 4);
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(cs + half);
  const f32x4 s1 = *reinterpret_cast<const f32x4*>(cs + half + 4);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float c = j < 4 ? c0[j & 3] : c1[j & 3], s = j < 4 ? s0[j & 3] : s1[j & 3];
    const float l = bf16_to_f32(static_cast<uint16_t>(lo[j]));
    const float h = bf16_to_f32(static_cast<uint16_t>(hi[j]));
    lo[j] = f32_to_bf16(__builtin_fmaf(l, c, -(h * s)));
    hi[j] = f32_to_bf16(__builtin_fmaf(h, c, l * s));
  }
}

}  // namespace dlbb
