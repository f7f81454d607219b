// Grouped-query single-query (decode) attention over the bf16 KV cache, gfx950 (MI355X, CDNA4).
//
// Contract. qkv is the step's fused activation [B, T, (H_q + 2 H_kv), D] bf16 (token row stride
// ld): the H_q query heads, then the H_kv key heads, then the H_kv value heads. Query head h uses
// KV head h / G, G = H_q / H_kv in {2, 4, 8, 16}; D in {64, 128}. k_cache / v_cache are
// [B, H_kv, L_max, D] bf16 contiguous (attn_decode.hip's cache with H = H_kv). `length` is one
// device int32 (a negative value is clamped to 0), or int32[B] for the *_seq forms, where
// length[b] < 0 is an empty slot: nothing loaded or stored, a zero output row.
//
//   kv_append_gqa_kernel        K / V rows of T >= 1 tokens -> cache positions [len_b, len_b + T),
//                               16-byte loads and stores, positions >= L_max dropped on the device.
//   attn_decode_gqa_split_kernel  T = 1. The caller has appended first and `length` is not
//                               advanced (attn_prefill.hip's contract): query head h of row b
//                               attends cache positions 0 .. min(len_b, L_max - 1) of KV head
//                               h / G; every key and value comes from the cache. Grid (n_chunks,
//                               H_kv, B): workgroup (c, kvh, b) handles ALL G query heads of its
//                               KV head over keys [c chunk, min((c + 1) chunk, L)) and writes one
//                               fp32 partial (m, l, o[D]) per query head to the workspace
//                               [B, H_q, n_chunks, D + 2] (attn_decode.hip's layout with H = H_q).
//   attn_decode_gqa_combine_kernel  one workgroup per (b, h_q): merges the live chunks' partials
//                               in chunk order and writes bf16 [B, 1, H_q * D], heads interleaved.
//
// The split kernel reads every K / V row ONCE for the G heads that share it; with G queries per
// key row the score and PV products are small matrix products on v_mfma_f32_16x16x32_bf16.
//   * The 4 waves of a workgroup split the chunk's KEYS (a quarter each, so `chunk` must be a
//     multiple of 4 x 32), not the queries; a wave walks its quarter in steps of 32 keys.
//   * Q of the G heads is loaded once as the B operand (D x 16): lane (n = lane % 16, g = lane /
//     16) holds Q[head n][32 ks + 8 g + j]. Columns n >= G are padding: they load head G - 1
//     (finite values) and are never stored.
//   * Scores S^T[16 keys x 16 heads] = K[16 x D] Q^T, two 16-key groups per step. The A operand
//     goes from global memory straight into VGPRs: lane (r = lane % 16, g) loads the 16 bytes
//     d = 32 ks + 8 g .. + 8 of key row r, so the four lanes of a row read 64 contiguous bytes per
//     instruction, and Q uses the same contraction order. K needs no LDS. The K fragments of step
//     i + 1 are loaded while step i is computed (two register sets, the loop is unrolled by two).
//   * Online softmax per head column in the MFMA C layout: a lane holds keys 4 g + i of both
//     groups for column n, so a column's max is 8 registers and two cross-lane steps (xor 16,
//     32). fp32 running m, l per column; "no key" is the finite -1e30 and the running max starts
//     at half of it (scaled), as in attn_prefill.hip: no inf - inf, a masked key gives p = 0.
//   * PV: O^T[D x 16 heads] += V^T[D x 32 keys] P^T[32 keys x 16]. The B operand's k index
//     8 g + j stands for key 4 g + j (j < 4) or 16 + 4 g + j - 4 (j >= 4): under this fixed
//     permutation the 8 probabilities a lane holds after the two score MFMAs ARE its B fragment,
//     no cross-lane movement. V needs the transpose: the wave's 32 V rows are staged into a
//     wave-private LDS image by LDS-DMA (attn_glds16; 16-byte chunk c of row r in slot
//     c ^ vswz_d(r), attn_tile.h) and read back with ds_read_b64_tr_b16 under the same key
//     permutation (rows 4 g + u and 16 + 4 g + u). Two images per wave: the DMA of step i + 1
//     flies while step i is computed. The images are wave-private, so the key loop has no
//     workgroup barrier, only s_waitcnt. LDS: 2 x 32 rows x 2 D bytes per wave, 64 KiB per
//     workgroup at D = 128, 32 KiB at D = 64.
//   * Edges. Only the step that holds the wave's last key is masked (a per-lane threshold on the
//     key index, the test is wave-uniform). Rows at or past the wave's end are never loaded: they
//     are redirected to its last live row and their scores masked (stale rows may hold NaN, and
//     0 * NaN is NaN in the PV product). A wave with no key in the chunk keeps the partial of no
//     keys.
//   * End of chunk: the four waves' (m, l, o) per head go through LDS (the V images, after a
//     barrier) and are merged in wave order; no atomics, no tickets: bit-identical from run to
//     run. PerSeq changes only where L comes from, so row b of a ragged launch has the bits of a
//     batch-1 shared-length launch at length[b].
//
// Sliding window (the Win instantiations, dlbb_attn_decode_gqa_win*): the query attends the last
// W keys, itself included: rows [lo, L) with L as above and lo = max(0, L - W). The chunks are
// laid from lo, not from 0: workgroup (c, kvh, b) owns [lo + c chunk, min(lo + (c + 1) chunk, L)),
// n_chunks = ceil(min(len_bound, W) / chunk), the combine merges ceil((L - lo) / chunk) partials.
// The grid, the live part of the workspace and the bytes read depend on the window, not on the
// context length, and no row below lo is addressed. Contract: for a given (b, kvh, c, lo, L) the
// workgroup does the arithmetic of the unwindowed kernel at (c, L - lo) on rows shifted by lo, in
// the same order (K rows are loaded one by one and V rows by per-row DMA, so the shift costs no
// alignment). With W >= L the result has the bits of the unwindowed launch at the same chunk;
// when the window bites, those of an unwindowed launch on a cache holding keys [lo, L) at
// positions 0 .. L - lo - 1.
//
// Rotary position embedding (the Rope instantiations, dlbb_*_gqa*_rope*; the table and the rotation
// are attn_tile.h's rope_rotate8). K is rotated ONCE, on its way into the cache, at its own cache
// position; V is stored untouched. Q is rotated in registers right after the split kernel's loads:
// the lane that holds Q[head][32 ks + 8 g + j] holds the partner column 32 (ks + D / 64) + 8 g + j
// too, so the rotation needs no other lane, no LDS and no launch of its own. The table row is
// L - 1, the ABSOLUTE cache position of the decoded token (under a window too, where the keys are
// addressed from lo); every chunk's workgroup rotates its copy of Q at that same row, and the
// padding columns rotate head G - 1 (finite). Nothing in the key loop differs and the combine
// kernel is the unroped one. The table must have at least L_max rows (the caller's check).
#include "attn_tile.h"
#include "common.h"

namespace dlbb {

namespace {

constexpr int kGqaThreads = 256;
constexpr int kGqaWaves = kGqaThreads / kWave;
constexpr int kGqaStep = 32;             // keys per wave step
constexpr float kGqaNegBig = -1.0e30f;   // raw score of a masked key: finite

struct GqaAppendArgs {
  const uint16_t* qkv;   // [B, T, H_q + 2 H_kv, D], token row stride ld
  uint16_t* k_cache;     // [B, H_kv, L_max, D]
  uint16_t* v_cache;
  const int* length;
  int64_t ld;
  int B, T, Hq, Hkv, D, L_max;
  const float* rope;     // the Rope kernel: cos | sin rows [>= L_max, D] fp32
};

// one 16-byte vector per thread step: (b, t, k|v, h_kv, piece). PerSeq: length[b], not *length
template <bool PerSeq>
__global__ __launch_bounds__(256) void kv_append_gqa_kernel(GqaAppendArgs a) {
  [[maybe_unused]] const int len0 = PerSeq ? 0 : *a.length;
  const int vpr = a.D / 8;                                  // vectors per head row
  const int64_t per_tok = 2LL * a.Hkv * vpr;
  const int64_t total = static_cast<int64_t>(a.B) * a.T * per_tok;
  const int64_t step = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += step) {
    const int64_t tok = i / per_tok;
    const int r = static_cast<int>(i - tok * per_tok);      // (k|v, h, piece)
    const int b = static_cast<int>(tok / a.T), t = static_cast<int>(tok - (int64_t)b * a.T);
    const int kv = r / (a.Hkv * vpr);
    const int hp = r - kv * a.Hkv * vpr;                    // h * vpr + piece
    const int h = hp / vpr, piece = hp - h * vpr;
    int len;
    if constexpr (PerSeq) len = a.length[b];
    else len = len0;
    const int64_t pos = static_cast<int64_t>(len) + t;
    if (len < 0 || pos >= a.L_max) continue;                // device-side guard: never past the cache
    const u16x8 val = *reinterpret_cast<const u16x8*>(
        a.qkv + (static_cast<int64_t>(b) * a.T + t) * a.ld +
        static_cast<int64_t>(a.Hq + kv * a.Hkv) * a.D + hp * 8);
    uint16_t* dst = (kv ? a.v_cache : a.k_cache) +
                    ((static_cast<int64_t>(b) * a.Hkv + h) * a.L_max + pos) * a.D + piece * 8;
    *reinterpret_cast<u16x8*>(dst) = val;
  }
}

// The same with K rotated at its cache position (V is copied as above). A K work item is a PAIR:
// the 16-byte piece `piece` of the row's low half and the matching piece of its high half, with
// the 8 cos and 8 sin floats of the position: D / 16 K items and D / 8 V items per (b, t, h_kv).
// The guards come first: an empty slot or a position past the cache reads no K, V or table row
template <bool PerSeq>
__global__ __launch_bounds__(256) void kv_append_gqa_rope_kernel(GqaAppendArgs a) {
  [[maybe_unused]] const int len0 = PerSeq ? 0 : *a.length;
  const int vpr = a.D / 8, kpr = a.D / 16;                  // V / K items per head row
  const int kitems = a.Hkv * kpr;
  const int64_t per_tok = kitems + static_cast<int64_t>(a.Hkv) * vpr;
  const int64_t total = static_cast<int64_t>(a.B) * a.T * per_tok;
  const int64_t step = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += step) {
    const int64_t tok = i / per_tok;
    const int r = static_cast<int>(i - tok * per_tok);      // K: (h, pair); then V: (h, piece)
    const int b = static_cast<int>(tok / a.T), t = static_cast<int>(tok - (int64_t)b * a.T);
    int len;
    if constexpr (PerSeq) len = a.length[b];
    else len = len0;
    const int64_t pos = static_cast<int64_t>(len) + t;
    if (len < 0 || pos >= a.L_max) continue;                // device-side guard: never past the cache
    const uint16_t* src = a.qkv + (static_cast<int64_t>(b) * a.T + t) * a.ld +
                          static_cast<int64_t>(a.Hq) * a.D;  // the token's K heads, then its V heads
    if (r < kitems) {
      const int h = r / kpr, piece = r - h * kpr;
      const uint16_t* sp = src + h * a.D + piece * 8;
      u16x8 lo = *reinterpret_cast<const u16x8*>(sp);
      u16x8 hi = *reinterpret_cast<const u16x8*>(sp + a.D / 2);
      rope_rotate8(lo, hi, a.rope + pos * a.D + piece * 8, a.D / 2);
      uint16_t* dst = a.k_cache +
                      ((static_cast<int64_t>(b) * a.Hkv + h) * a.L_max + pos) * a.D + piece * 8;
      *reinterpret_cast<u16x8*>(dst) = lo;
      *reinterpret_cast<u16x8*>(dst + a.D / 2) = hi;
    } else {
      const int hp = r - kitems;                            // h * vpr + piece
      const int h = hp / vpr, piece = hp - h * vpr;
      const u16x8 val = *reinterpret_cast<const u16x8*>(src + a.Hkv * a.D + hp * 8);
      uint16_t* dst = a.v_cache +
                      ((static_cast<int64_t>(b) * a.Hkv + h) * a.L_max + pos) * a.D + piece * 8;
      *reinterpret_cast<u16x8*>(dst) = val;
    }
  }
}

struct GqaArgs {
  const uint16_t* qkv;      // [B, 1, H_q + 2 H_kv, D], batch row stride ld
  const uint16_t* k_cache;  // [B, H_kv, L_max, D]
  const uint16_t* v_cache;
  const int* length;
  float* ws;                // [B, H_q, n_chunks, D + 2]: m, l, o[D]
  uint16_t* out;            // [B, 1, H_q, D], batch row stride ldo
  int64_t ld, ldo;
  int B, Hq, Hkv, G, L_max, chunk, n_chunks;
  float scale_log2;         // log2(e) * scale
  int window;               // Win kernels: keys a query attends, 1 .. L_max
  const float* rope;        // Rope kernels: cos | sin rows [>= L_max, D] fp32
};

// keys row b attends: positions 0 .. min(len, L_max - 1) (the token was appended at `len`).
// PerSeq: a negative length is an empty slot, 0 keys, `empty` set
template <bool PerSeq>
__device__ __forceinline__ int gqa_keys(const GqaArgs& a, int b, bool& empty) {
  int len;
  empty = false;
  if constexpr (PerSeq) {
    len = a.length[b];
    if (len < 0) {
      empty = true;
      return 0;
    }
  } else {
    len = *a.length;
    if (len < 0) len = 0;
  }
  return len < a.L_max ? len + 1 : a.L_max;
}

// first key of a window of a.window keys that ends at L
__device__ __forceinline__ int gqa_window_lo(const GqaArgs& a, int L) {
  return L > a.window ? L - a.window : 0;
}

template <int D, bool PerSeq, bool Win, bool Rope>
__global__ void __launch_bounds__(kGqaThreads, 2) attn_decode_gqa_split_kernel(GqaArgs a) {
  constexpr int ROW = 2 * D;                 // bytes of a V row
  constexpr int RPI = 1024 / ROW;            // rows per DMA wave-instruction
  constexpr int NDMA = kGqaStep / RPI;       // DMA wave-instructions per image
  constexpr int NKS = D / 32;                // k-steps of S^T = K Q^T
  constexpr int NDB = D / 16;                // 16-dim blocks of O^T
  constexpr int VBUF = kGqaStep * ROW;       // one V image: 8 KiB at D = 128, 4 KiB at D = 64
  constexpr int RED = D + 2;                 // floats of one (wave, head) partial
  static_assert(kGqaWaves * 16 * RED * 4 <= kGqaWaves * 2 * VBUF, "the merge reuses the images");
  __shared__ __attribute__((aligned(16))) char smem[kGqaWaves * 2 * VBUF];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 15, g = lane >> 4;    // MFMA column (head) / k-group of the lane
  const int c = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  bool empty;
  const int L = gqa_keys<PerSeq>(a, b, empty);
  int lo = 0;                                // Win: the chunks are laid from the window's first key
  if constexpr (Win) lo = gqa_window_lo(a, L);
  if (c * a.chunk >= L - lo) return;         // dead chunk (every chunk of an empty slot): no K / V
                                             // read, no partial written
  const int c0 = lo + c * a.chunk;
  const int c1 = min(c0 + a.chunk, L);
  const int quarter = a.chunk / kGqaWaves;   // a multiple of kGqaStep (checked by the launcher)
  const int w0 = c0 + wave * quarter;        // this wave's keys [w0, w1); none when w1 <= w0
  const int w1 = min(w0 + quarter, c1);
  const int nst = w1 > w0 ? (w1 - w0 + kGqaStep - 1) / kGqaStep : 0;

  // Q fragments (B operand): lane holds Q[kvh G + min(n, G - 1)][32 ks + 8 g + j]
  bf16x8 qf[NKS];
  {
    const int hq = kvh * a.G + (n < a.G ? n : a.G - 1);
    const uint16_t* qp = a.qkv + static_cast<int64_t>(b) * a.ld + static_cast<int64_t>(hq) * D + 8 * g;
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + 32 * ks);
  }
  // Rope: k-step ks holds the low-half columns 32 ks + 8 g + j, k-step ks + NKS / 2 their partners;
  // table row L - 1 is the token's absolute position (not L - 1 - lo), < L_max
  if constexpr (Rope) {
    const float* cs = a.rope + static_cast<int64_t>(L - 1) * D + 8 * g;
#pragma unroll
    for (int ks = 0; ks < NKS / 2; ++ks) rope_rotate8(qf[ks], qf[ks + NKS / 2], cs + 32 * ks, D / 2);
  }
  const int64_t rows = (static_cast<int64_t>(b) * a.Hkv + kvh) * a.L_max;
  const uint16_t* kc = a.k_cache + rows * D + 8 * g;   // the lane's 8 columns of row 0
  const uint16_t* vc = a.v_cache + rows * D;

  // K fragments of the 32 keys from kb (A operand): group t, lane row n -> key kb + 16 t + n; a
  // key at or past w1 re-reads the wave's last live row (its score is masked)
  auto load_k = [&](int kb, bf16x8 (&kf)[2][NKS]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      int row = kb + 16 * t + n;
      row = row < w1 ? row : w1 - 1;
      const uint16_t* p = kc + static_cast<int64_t>(row) * D;
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) kf[t][ks] = *reinterpret_cast<const bf16x8*>(p + 32 * ks);
    }
  };

  // V image of the 32 keys from kb into the wave's buffer `buf`: DMA instruction i carries image
  // rows i RPI .. + RPI, the lane row r_in of them, LDS slot `slot` <- chunk slot ^ swz(row)
  char* vimg = smem + wave * 2 * VBUF;
  const int r_in = lane / (ROW / 16), slot = lane % (ROW / 16);
  auto stage_v = [&](int kb, int buf) {
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
      const int rt = i * RPI + r_in;
      int row = kb + rt;
      row = row < w1 ? row : w1 - 1;
      attn_glds16(vc + static_cast<int64_t>(row) * D + (slot ^ vswz_d<D>(rt)) * 8,
                  vimg + buf * VBUF + i * RPI * ROW);
    }
  };

  // transposed-read lane role inside a 16-lane group: the lane addresses 4 consecutive d of image
  // row 4 g + tq (and 16 + 4 g + tq) and receives column n of rows 4 g + u; swz depends on tq only
  const int tq = n >> 2, tp = n & 3;
  const int vsw = vswz_d<D>(tq), tph = tp >> 1;
  const char* vrd = vimg + (4 * g + tq) * ROW + (tp & 1) * 8;

  f32x4 o[NDB];                              // O^T: o[db][i] = O[d = 16 db + 4 g + i][head n]
#pragma unroll
  for (int db = 0; db < NDB; ++db) o[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = 0.5f * kGqaNegBig * a.scale_log2, l = 0.f;

  // one 32-key step on buffer `cur` with the fragments kf; loads step it + 1 into kn / cur ^ 1
  auto step = [&](int it, int cur, const bf16x8 (&kf)[2][NKS], bf16x8 (&kn)[2][NKS]) {
    const int kb = w0 + it * kGqaStep;
    // everything issued one step ago has landed: K of this step in kf, its V image in `cur`; the
    // transposed reads of the step before (of buffer cur ^ 1) were waited for before their MFMAs
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (it + 1 < nst) {
      load_k(kb + kGqaStep, kn);
      stage_v(kb + kGqaStep, cur ^ 1);
    }
    f32x4 s0{0.f, 0.f, 0.f, 0.f}, s1{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
      s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[0][ks], qf[ks], s0, 0, 0, 0);
      s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[1][ks], qf[ks], s1, 0, 0, 0);
    }
    if (kb + kGqaStep > w1) {                // wave-uniform: the step holding the last key
      // key(s0, i) = kb + 4 g + i, key(s1, i) = kb + 16 + 4 g + i: one per-lane threshold
      const int th = w1 - kb - 4 * g;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i >= th) s0[i] = kGqaNegBig;
        if (16 + i >= th) s1[i] = kGqaNegBig;
      }
    }
    float mx = fmaxf(fmaxf(fmaxf(s0[0], s0[1]), fmaxf(s0[2], s0[3])),
                     fmaxf(fmaxf(s1[0], s1[1]), fmaxf(s1[2], s1[3])));
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // the column's max of the RAW scores (scale > 0)
    const float mn = fmaxf(m, mx * a.scale_log2);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    m = mn;
    float ls = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s0[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s0[i], a.scale_log2, -mn));
      s1[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s1[i], a.scale_log2, -mn));
      ls += s0[i] + s1[i];
    }
    l = l * alpha + ls;
    if (__any(alpha != 1.f)) {               // wave-uniform skip when no max moved
#pragma unroll
      for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int i = 0; i < 4; ++i) o[db][i] *= alpha;
    }
    // P^T fragment: k index 8 g + j <-> key 4 g + j (j < 4), 16 + 4 g + j - 4 (j >= 4)
    bf16x8 pf;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pf[i] = __builtin_bit_cast(short, static_cast<__bf16>(s0[i]));
      pf[4 + i] = __builtin_bit_cast(short, static_cast<__bf16>(s1[i]));
    }
    // O^T += V^T P^T, four 16-dim blocks per batch of transposed reads
    const char* vb = vrd + cur * VBUF;
#pragma unroll
    for (int d0 = 0; d0 < NDB; d0 += 4) {
      i16x4 lo[4], hi[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const char* p = vb + (((2 * (d0 + u) + tph) ^ vsw) << 4);
        lo[u] = ds_read_tr16<0>(p);
        hi[u] = ds_read_tr16<16 * ROW>(p);
      }
      tr_wait(lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        bf16x8 vf;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          vf[j] = lo[u][j];
          vf[4 + j] = hi[u][j];
        }
        o[d0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[d0 + u], 0, 0, 0);
      }
    }
  };

  bf16x8 ka[2][NKS], kb2[2][NKS];
  if (nst > 0) {
    load_k(w0, ka);
    stage_v(w0, 0);
  }
  for (int it = 0; it < nst; it += 2) {
    step(it, 0, ka, kb2);
    if (it + 1 < nst) step(it + 1, 1, kb2, ka);
  }

  // ---- merge: l over the column's four lanes, then the four waves through LDS in wave order
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  __syncthreads();                           // every wave is done with its images
  float* red = reinterpret_cast<float*>(smem);
  if (n < a.G) {
    float* p = red + (wave * 16 + n) * RED;
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int i = 0; i < 4; ++i) p[2 + 16 * db + 4 * g + i] = o[db][i];
    if (g == 0) {
      p[0] = m;
      p[1] = l;
    }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < a.G * D; idx += kGqaThreads) {
    const int hn = idx / D, d = idx - hn * D;
    const float* p = red + hn * RED;
    float mw = p[0];
#pragma unroll
    for (int w = 1; w < kGqaWaves; ++w) mw = fmaxf(mw, p[w * 16 * RED]);
    float lw = 0.f, ow = 0.f;
#pragma unroll
    for (int w = 0; w < kGqaWaves; ++w) {
      const float f = __builtin_amdgcn_exp2f(p[w * 16 * RED] - mw);
      lw = __builtin_fmaf(p[w * 16 * RED + 1], f, lw);
      ow = __builtin_fmaf(p[w * 16 * RED + 2 + d], f, ow);
    }
    float* q = a.ws +
               ((static_cast<int64_t>(b) * a.Hq + kvh * a.G + hn) * a.n_chunks + c) * (D + 2);
    q[2 + d] = ow;
    if (d == 0) {
      q[0] = mw;
      q[1] = lw;
    }
  }
}

// grid (H_q, B), D threads: thread d owns output column d of query head h
template <int D, bool PerSeq, bool Win>
__global__ __launch_bounds__(D) void attn_decode_gqa_combine_kernel(GqaArgs a) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  bool empty;
  const int L = gqa_keys<PerSeq>(a, b, empty);
  uint16_t* op = a.out + static_cast<int64_t>(b) * a.ldo + h * D + d;
  if (empty) {                                     // an empty slot has no partials: zeros
    *op = 0;
    return;
  }
  int keys = L;                                    // Win: the chunks hold the window's keys only
  if constexpr (Win) keys = L - gqa_window_lo(a, L);
  const int live = min((keys + a.chunk - 1) / a.chunk, a.n_chunks);
  const float* p = a.ws + (static_cast<int64_t>(b) * a.Hq + h) * a.n_chunks * (D + 2);
  float mx = kGqaNegBig;
#pragma unroll 4
  for (int c = 0; c < live; ++c) mx = fmaxf(mx, p[static_cast<int64_t>(c) * (D + 2)]);
  float lsum = 0.f, acc = 0.f;
#pragma unroll 4
  for (int c = 0; c < live; ++c) {                 // chunk order: fixed summation order
    const float* pc = p + static_cast<int64_t>(c) * (D + 2);
    const float f = __builtin_amdgcn_exp2f(pc[0] - mx);
    lsum = __builtin_fmaf(pc[1], f, lsum);
    acc = __builtin_fmaf(pc[2 + d], f, acc);
  }
  *op = f32_to_bf16(acc / lsum);
}

bool mis(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

// the supported range: D in {64, 128}, G = H_q / H_kv in {2, 4, 8, 16}
bool gqa_range_ok(int Hq, int Hkv, int D) {
  if (D != 64 && D != 128) return false;
  if (Hq <= 0 || Hkv <= 0 || Hq % Hkv) return false;
  const int G = Hq / Hkv;
  return G == 2 || G == 4 || G == 8 || G == 16;
}

// what the entry points ask of qkv, the cache geometry and `length` (attn_decode.hip's checks with
// the row width of the grouped layout)
bool gqa_qkv_cache_ok(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache,
                      const void* length, int Hq, int Hkv, int D, int L_max) {
  if (L_max <= 0 || ld % 8 || ld < static_cast<int64_t>(Hq + 2 * Hkv) * D) return false;
  if (!qkv || !k_cache || !v_cache || !length || mis(length, 4)) return false;
  return !(mis(qkv, 16) || mis(k_cache, 16) || mis(v_cache, 16));
}

// Rope: `rope` is the cos | sin table (fp32 [>= L_max, D], 16-byte aligned), K is stored rotated
template <bool PerSeq, bool Rope = false>
int gqa_append_launch(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                      const void* length, int B, int T, int Hq, int Hkv, int D, int L_max,
                      hipStream_t stream, const void* rope = nullptr) {
  if (!gqa_range_ok(Hq, Hkv, D)) return hipErrorInvalidValue;
  if (Rope && (!rope || mis(rope, 16))) return hipErrorInvalidValue;
  if (B <= 0 || T <= 0) return hipSuccess;
  if (!gqa_qkv_cache_ok(qkv, ld, k_cache, v_cache, length, Hq, Hkv, D, L_max))
    return hipErrorInvalidValue;
  GqaAppendArgs a{static_cast<const uint16_t*>(qkv), static_cast<uint16_t*>(k_cache),
                  static_cast<uint16_t*>(v_cache), static_cast<const int*>(length), ld, B, T, Hq,
                  Hkv, D, L_max, static_cast<const float*>(rope)};
  if constexpr (Rope) {
    const int64_t items = static_cast<int64_t>(B) * T * Hkv * (D / 16 + D / 8);
    hipLaunchKernelGGL((kv_append_gqa_rope_kernel<PerSeq>), dim3(stream_grid(items, 256)),
                       dim3(256), 0, stream, a);
  } else {
    const int64_t vecs = static_cast<int64_t>(B) * T * 2 * Hkv * (D / 8);
    hipLaunchKernelGGL((kv_append_gqa_kernel<PerSeq>), dim3(stream_grid(vecs, 256)), dim3(256), 0,
                       stream, a);
  }
  return hipGetLastError();
}

// Win: `window` keys per query (>= 1, clamped to L_max: a window at or over L_max is no window).
// Rope: `rope` is the cos | sin table (fp32 [>= L_max, D], 16-byte aligned), Q is rotated at L - 1
template <bool PerSeq, bool Win = false, bool Rope = false>
int gqa_decode_launch(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache,
                      const void* length, void* ws, void* out, int64_t ldo, int B, int Hq,
                      int Hkv, int D, int L_max, int len_bound, int chunk, float scale,
                      hipStream_t stream, int window = 0, const void* rope = nullptr) {
  if (!gqa_range_ok(Hq, Hkv, D)) return hipErrorInvalidValue;
  if (Rope && (!rope || mis(rope, 16))) return hipErrorInvalidValue;
  if (B <= 0) return hipSuccess;
  if (!gqa_qkv_cache_ok(qkv, ld, k_cache, v_cache, length, Hq, Hkv, D, L_max))
    return hipErrorInvalidValue;
  if (chunk <= 0 || chunk % (kGqaWaves * kGqaStep) || len_bound <= 0) return hipErrorInvalidValue;
  if (!ws || mis(ws, 4) || !out || mis(out, 2) || ldo < static_cast<int64_t>(Hq) * D)
    return hipErrorInvalidValue;
  if (!(scale > 0.f) || Hq > 65535 || B > 65535) return hipErrorInvalidValue;
  if (Win && window < 1) return hipErrorInvalidValue;
  if (len_bound > L_max) len_bound = L_max;
  if (window > L_max) window = L_max;
  if (Win && len_bound > window) len_bound = window;   // the grid covers the window's keys only
  const int n_chunks = (len_bound + chunk - 1) / chunk;
  GqaArgs a{static_cast<const uint16_t*>(qkv), static_cast<const uint16_t*>(k_cache),
            static_cast<const uint16_t*>(v_cache), static_cast<const int*>(length),
            static_cast<float*>(ws), static_cast<uint16_t*>(out), ld, ldo, B, Hq, Hkv, Hq / Hkv,
            L_max, chunk, n_chunks, scale * 1.4426950408889634f, window,
            static_cast<const float*>(rope)};
  const dim3 gs(n_chunks, Hkv, B), gc(Hq, B);
  if (D == 64) {
    hipLaunchKernelGGL((attn_decode_gqa_split_kernel<64, PerSeq, Win, Rope>), gs, dim3(kGqaThreads), 0,
                       stream, a);
    hipLaunchKernelGGL((attn_decode_gqa_combine_kernel<64, PerSeq, Win>), gc, dim3(64), 0, stream, a);
  } else {
    hipLaunchKernelGGL((attn_decode_gqa_split_kernel<128, PerSeq, Win, Rope>), gs, dim3(kGqaThreads), 0,
                       stream, a);
    hipLaunchKernelGGL((attn_decode_gqa_combine_kernel<128, PerSeq, Win>), gc, dim3(128), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace

}  // namespace dlbb

using namespace dlbb;

// qkv [B, T, H_q + 2 H_kv, D] bf16 (token row stride ld elements: H_q query heads, H_kv key
// heads, H_kv value heads); k_cache / v_cache [B, H_kv, L_max, D] bf16 contiguous; length: ONE
// device int32. The K / V rows of every token go to cache positions [*length, *length + T);
// positions >= L_max are dropped on the device. D outside {64, 128} or H_q / H_kv outside
// {2, 4, 8, 16} (or not whole), a null or misaligned pointer or ld too small return
// hipErrorInvalidValue before any launch.
DLBB_API int dlbb_kv_append_gqa(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                const void* length, int B, int T, int Hq, int Hkv, int D,
                                int L_max, hipStream_t stream) {
  return gqa_append_launch<false>(qkv, ld, k_cache, v_cache, length, B, T, Hq, Hkv, D, L_max,
                                  stream);
}

// Per-sequence lengths: length is device int32[B]; row b's tokens go to positions [length[b],
// length[b] + T), nothing is written for a row with length[b] < 0.
DLBB_API int dlbb_kv_append_gqa_seq(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                    const void* length, int B, int T, int Hq, int Hkv, int D,
                                    int L_max, hipStream_t stream) {
  return gqa_append_launch<true>(qkv, ld, k_cache, v_cache, length, B, T, Hq, Hkv, D, L_max,
                                 stream);
}

// One decode step of grouped-query attention: qkv [B, 1, H_q + 2 H_kv, D] (batch row stride ld),
// the cache as above with the token's K / V already appended at *length (dlbb_kv_append_gqa) and
// *length not advanced; query head h attends positions 0 .. min(*length, L_max - 1) of KV head
// h / (H_q / H_kv). out [B, 1, H_q, D] bf16 (batch row stride ldo). ws: fp32 [B, H_q, n_chunks,
// D + 2], n_chunks = ceil(min(len_bound, L_max) / chunk); len_bound is the host's upper bound of
// *length + 1; chunk must be a multiple of 128 keys (4 waves x 32-key steps).
DLBB_API int dlbb_attn_decode_gqa(const void* qkv, int64_t ld, const void* k_cache,
                                  const void* v_cache, const void* length, void* ws, void* out,
                                  int64_t ldo, int B, int Hq, int Hkv, int D, int L_max,
                                  int len_bound, int chunk, float scale, hipStream_t stream) {
  return gqa_decode_launch<false>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B, Hq, Hkv, D,
                                  L_max, len_bound, chunk, scale, stream);
}

// The same with per-sequence lengths: length is device int32[B]; a row with length[b] < 0 is an
// empty slot: nothing read, its output row is zeros. len_bound bounds max_b length[b] + 1.
DLBB_API int dlbb_attn_decode_gqa_seq(const void* qkv, int64_t ld, const void* k_cache,
                                      const void* v_cache, const void* length, void* ws,
                                      void* out, int64_t ldo, int B, int Hq, int Hkv, int D,
                                      int L_max, int len_bound, int chunk, float scale,
                                      hipStream_t stream) {
  return gqa_decode_launch<true>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B, Hq, Hkv, D,
                                 L_max, len_bound, chunk, scale, stream);
}

// Sliding window: dlbb_attn_decode_gqa with `window` >= 1 keys per query. Query head h attends
// positions max(0, L - window) .. L - 1, L = min(*length, L_max - 1) + 1 (its own token
// included); a window at or over L_max is no window. ws: fp32 [B, H_q, n_chunks, D + 2] with
// n_chunks = ceil(min(len_bound, window, L_max) / chunk): the chunks are laid from the window's
// first key, so the grid and the workspace do not grow with the context. window < 1 returns
// hipErrorInvalidValue before any launch.
DLBB_API int dlbb_attn_decode_gqa_win(const void* qkv, int64_t ld, const void* k_cache,
                                      const void* v_cache, const void* length, void* ws,
                                      void* out, int64_t ldo, int B, int Hq, int Hkv, int D,
                                      int L_max, int len_bound, int chunk, int window,
                                      float scale, hipStream_t stream) {
  return gqa_decode_launch<false, true>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B, Hq,
                                        Hkv, D, L_max, len_bound, chunk, scale, stream, window);
}

// The same with per-sequence lengths (dlbb_attn_decode_gqa_seq's rules): row b attends the last
// `window` of its own length[b] + 1 keys.
DLBB_API int dlbb_attn_decode_gqa_win_seq(const void* qkv, int64_t ld, const void* k_cache,
                                          const void* v_cache, const void* length, void* ws,
                                          void* out, int64_t ldo, int B, int Hq, int Hkv, int D,
                                          int L_max, int len_bound, int chunk, int window,
                                          float scale, hipStream_t stream) {
  return gqa_decode_launch<true, true>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B, Hq,
                                       Hkv, D, L_max, len_bound, chunk, scale, stream, window);
}

// The rotary forms (the file header, "Rotary position embedding"): the entry points above with
// `rope`, the cos | sin table (fp32 [P >= L_max, D] contiguous, 16-byte aligned; row p: cos of
// cache position p in [0, D / 2), sin in [D / 2, D)), after `length`. A null or misaligned table
// returns hipErrorInvalidValue before any launch. dlbb_kv_append_gqa_rope* store each K row rotated
// at its own position *length + t (length[b] + t) and the V rows untouched.
DLBB_API int dlbb_kv_append_gqa_rope(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                     const void* length, const void* rope, int B, int T, int Hq,
                                     int Hkv, int D, int L_max, hipStream_t stream) {
  return gqa_append_launch<false, true>(qkv, ld, k_cache, v_cache, length, B, T, Hq, Hkv, D, L_max,
                                        stream, rope);
}

DLBB_API int dlbb_kv_append_gqa_rope_seq(const void* qkv, int64_t ld, void* k_cache,
                                         void* v_cache, const void* length, const void* rope,
                                         int B, int T, int Hq, int Hkv, int D, int L_max,
                                         hipStream_t stream) {
  return gqa_append_launch<true, true>(qkv, ld, k_cache, v_cache, length, B, T, Hq, Hkv, D, L_max,
                                       stream, rope);
}

// dlbb_attn_decode_gqa* with Q rotated at table row min(*length, L_max - 1), the position at which
// dlbb_kv_append_gqa_rope* stored the token's K; the cache must hold keys rotated with this table.
DLBB_API int dlbb_attn_decode_gqa_rope(const void* qkv, int64_t ld, const void* k_cache,
                                       const void* v_cache, const void* length, const void* rope,
                                       void* ws, void* out, int64_t ldo, int B, int Hq, int Hkv,
                                       int D, int L_max, int len_bound, int chunk, float scale,
                                       hipStream_t stream) {
  return gqa_decode_launch<false, false, true>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B,
                                               Hq, Hkv, D, L_max, len_bound, chunk, scale, stream,
                                               0, rope);
}

DLBB_API int dlbb_attn_decode_gqa_rope_seq(const void* qkv, int64_t ld, const void* k_cache,
                                           const void* v_cache, const void* length,
                                           const void* rope, void* ws, void* out, int64_t ldo,
                                           int B, int Hq, int Hkv, int D, int L_max, int len_bound,
                                           int chunk, float scale, hipStream_t stream) {
  return gqa_decode_launch<true, false, true>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B,
                                              Hq, Hkv, D, L_max, len_bound, chunk, scale, stream,
                                              0, rope);
}

// The windowed forms: the table row is still the token's absolute position, not its place in the
// window.
DLBB_API int dlbb_attn_decode_gqa_win_rope(const void* qkv, int64_t ld, const void* k_cache,
                                           const void* v_cache, const void* length,
                                           const void* rope, void* ws, void* out, int64_t ldo,
                                           int B, int Hq, int Hkv, int D, int L_max, int len_bound,
                                           int chunk, int window, float scale,
                                           hipStream_t stream) {
  return gqa_decode_launch<false, true, true>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B,
                                              Hq, Hkv, D, L_max, len_bound, chunk, scale, stream,
                                              window, rope);
}

DLBB_API int dlbb_attn_decode_gqa_win_rope_seq(const void* qkv, int64_t ld, const void* k_cache,
                                               const void* v_cache, const void* length,
                                               const void* rope, void* ws, void* out, int64_t ldo,
                                               int B, int Hq, int Hkv, int D, int L_max,
                                               int len_bound, int chunk, int window, float scale,
                                               hipStream_t stream) {
  return gqa_decode_launch<true, true, true>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B,
                                             Hq, Hkv, D, L_max, len_bound, chunk, scale, stream,
                                             window, rope);
}
