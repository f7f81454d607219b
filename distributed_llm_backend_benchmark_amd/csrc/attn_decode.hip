// Single-query (decode) attention over a KV cache, bf16 or FP8 (OCP e4m3fn), gfx950 (MI355X,
// CDNA4).
//
// Cache layout, per layer and rank: k_cache / v_cache [B, H, L_max, D], contiguous, so the key
// stream of one (b, h) is one contiguous run; `length` is ONE device int32 = tokens already
// cached, shared by the batch (and by every layer). Every kernel here reads it from device
// memory, so a step captured in a HIP graph replays for successive positions.
//
// Per-sequence lengths (the *_seq entry points): `length` is int32[B] and row b of every kernel
// uses length[b]; length[b] < 0 marks a slot that holds no sequence (nothing appended, its split
// workgroups exit before any load or store, the combine writes zeros to its output row). The
// kernels are the same templates with PerSeq = true: the work of a workgroup for a given
// (b, h, c, L) is that of the shared-length kernel, only where L comes from differs. The
// shared-length forms (PerSeq = false) are instantiations of their own, compiled as before.
//
// Paged caches (the *_paged entry points): K / V live in pools k_pool / v_pool [n_pages, H, P, D]
// (FP8: and k_scale / v_scale [n_pages, H, P]) shared by every batch row; the P rows of one
// (page, head) are one contiguous run. `block_table` is int32[B, max_pages], max_pages =
// ceil(L_max / P), one table for every layer: logical position t of row b lives in physical page
// block_table[b, t / P] at row t % P. P is a power of two in [16, 256] that divides `chunk`, so a
// chunk covers whole pages. `length` is always the per-sequence int32[B], and every *_seq rule
// holds; L_max is the logical cap. An entry outside [0, n_pages) is an UNMAPPED page and never
// becomes an address: a store to a position on it is dropped, a key on it below L is masked out
// of the softmax and its loads are redirected to a row of the chunk's first mapped page (as
// masked slots re-read a live row). The padded prefill relies on this rule. A chunk without any
// mapped page writes the partial of no keys (m = -1e30, l = 0, o = 0); a live row with no mapped
// key at all has no defined output. The kernels are the same templates with Paged = true: for a
// given (b, h, chunk, L) a workgroup does the arithmetic of the *_seq kernel in the same order,
// only the addresses differ, so with equal contents a row has the bits of the contiguous
// per-sequence launch. A workgroup reads its chunk's <= 64 table entries once (one load per lane
// of a wave, a ballot for the first mapped page) and keeps them in LDS; a key's page is one LDS
// read. The combine kernel never sees the table.
//
//   bf16 cache  rows of D bf16 (2 D bytes).
//   FP8 cache   rows of D e4m3fn bytes and k_scale / v_scale [B, H, L_max] fp32: one scale per
//               cached row, row ~= float(code) * scale (D + 4 bytes a row). A row is quantised
//               exactly as gemm_fp8.hip's row quantiser does (ops.fp8): amax == 0 -> scale 1,
//               bytes 0; otherwise inv = 448 / amax and scale = amax / 448 (IEEE fp32 divisions)
//               and code = cvt_pk_fp8_f32(float(x) * inv), round to nearest even.
//
//   kv_append_kernel           K / V rows of a fused qkv [B, T, 3, H, D] bf16 -> cache positions
//                              [length, length + T), 16-byte loads and stores.
//   kv_append_fp8_kernel       the same rows -> codes and scales. One row lives in D / 8 lanes: a
//                              16-byte load per lane, amax by shuffles, one convert pass, an
//                              8-byte store of codes per lane.
//   attn_decode_split_kernel   grid (n_chunks, H, B): workgroup (c, h, b) attends the one query
//                              of (b, h) over keys [c * chunk, min((c + 1) * chunk, L)),
//                              L = length + 1 (the cached tokens and the token being decoded),
//                              and writes the partial (m, l, o[D]) in fp32 to the workspace.
//   attn_decode_combine_kernel one workgroup per (b, h): merges the live chunks' partials in
//                              chunk order and writes bf16 [B, 1, H * D] (heads interleaved). It
//                              never reads the cache: one kernel for both formats.
//
// The split kernel is a bandwidth-bound read: K and V go from global memory straight into
// VGPRs, 16 bytes per lane — 8 bf16 or 16 codes, so D / 8 or D / 16 lanes per key (a wave reads
// 1 KiB of consecutive key rows per load instruction); the dot product is reduced over those
// lanes with shuffles. Each such group of lanes (a "slot") keeps an online softmax of its own
// over the keys it walks (fp32 running max m, sum l, and its 8 or 16 columns of o); slots are
// merged once at the end, inside the wave by shuffles and across the 4 waves through LDS, in a
// fixed order. No MFMA, no LDS staging of K / V, no atomics, no tickets: results are
// bit-identical from run to run.
//
// FP8 codes are widened in registers (v_cvt_pk_f32_fp8, exact); the dot product runs on the raw
// codes, the key's scale is folded into the score (s = dot * k_scale * scale_log2) and the
// value's into the weight (o += (p * v_scale) * code, l += p).
//
// `fused` = 1: the chunk that owns position `length` takes the new token's K / V from `qkv` and
// also writes them to the cache, so append + attend is one launch; 0: the caller appended first
// (dlbb_kv_append / dlbb_kv_append_fp8) and every key is read from the cache. With the FP8 cache
// the fused chunk quantises the token, stores codes + scales and attends to those codes, so the
// step's result is attention over the cache contents after the append, exactly.
#include "common.h"

namespace dlbb {

namespace {

constexpr int kDecThreads = 256;
constexpr int kDecUnroll = 4;          // keys in flight per slot (8 x 16 B loads per lane, + 8 scales)
constexpr float kDecNegBig = -1.0e30f; // "no key yet": finite, so no inf - inf in the merges
constexpr float kE4m3Max = 448.0f;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// 16 e4m3fn bytes (byte order) -> 16 floats, exactly
__device__ __forceinline__ void e4m3x16_to_f32(const u32x4& r, float (&v)[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(r[i]), false);
    const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(r[i]), true);
    v[4 * i] = lo[0];
    v[4 * i + 1] = lo[1];
    v[4 * i + 2] = hi[0];
    v[4 * i + 3] = hi[1];
  }
}

// 4 floats -> 4 e4m3fn bytes (byte order), round to nearest even
__device__ __forceinline__ uint32_t f32x4_to_e4m3(float f0, float f1, float f2, float f3) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, w, true);
  return static_cast<uint32_t>(w);
}

// the row's scale and the multiplier of its elements, from the row's amax
__device__ __forceinline__ void row_scale(float amax, float& inv, float& scale) {
  const bool zero = amax == 0.f;
  inv = zero ? 1.0f : kE4m3Max / amax;
  scale = zero ? 1.0f : amax / kE4m3Max;
}

struct KvAppendArgs {
  const uint16_t* qkv;   // [B, T, 3, H, D], token row stride ld
  uint16_t* k_cache;     // [B, H, L_max, D]
  uint16_t* v_cache;
  const int* length;
  int64_t ld;
  int B, T, H, D, L_max;
  // Paged (after the contiguous forms' fields, whose offsets stay): k_cache / v_cache are the pools
  const int* table;      // [B, tstride]
  int64_t tstride;
  int n_pages, psh;      // P = 1 << psh
};

// row of a pool [n_pages, H, P, D] that holds logical position `pos` of head h in page pg
__device__ __forceinline__ int64_t pool_row(int pg, int H, int h, int psh, int64_t pos) {
  return ((static_cast<int64_t>(pg) * H + h) << psh) + (pos & ((1 << psh) - 1));
}

// the pool row of logical position `pos` of (b, h), -1 when its page is not mapped
__device__ __forceinline__ int64_t paged_row(const int* table, int64_t tstride, int n_pages,
                                             int psh, int H, int b, int h, int64_t pos) {
  const int pg = table[b * tstride + (pos >> psh)];
  if (pg < 0 || pg >= n_pages) return -1;
  return pool_row(pg, H, h, psh, pos);
}

// one 16-byte vector per thread step: (b, t, k|v, h, piece). PerSeq: length[b], not *length.
// Paged: the destination row comes through the block table, an unmapped one is dropped
template <bool PerSeq, bool Paged>
__global__ __launch_bounds__(256) void kv_append_kernel(KvAppendArgs a) {
  [[maybe_unused]] const int len0 = PerSeq ? 0 : *a.length;
  const int vpr = a.D / 8;                                  // vectors per head row
  const int64_t per_tok = 2LL * a.H * vpr;
  const int64_t total = static_cast<int64_t>(a.B) * a.T * per_tok;
  const int64_t step = static_cast<int64_t>(gridDim.x) * blockDim.x;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += step) {
    const int64_t tok = i / per_tok;
    const int r = static_cast<int>(i - tok * per_tok);      // (k|v, h, piece)
    const int b = static_cast<int>(tok / a.T), t = static_cast<int>(tok - (int64_t)b * a.T);
    const int kv = r / (a.H * vpr);
    const int hp = r - kv * a.H * vpr;                      // h * vpr + piece
    const int h = hp / vpr, piece = hp - h * vpr;
    int len;
    if constexpr (PerSeq) len = a.length[b];
    else len = len0;
    const int64_t pos = static_cast<int64_t>(len) + t;
    if (len < 0 || pos >= a.L_max) continue;                // device-side guard: never past the cache
    const u16x8 val = *reinterpret_cast<const u16x8*>(
        a.qkv + (static_cast<int64_t>(b) * a.T + t) * a.ld + static_cast<int64_t>(1 + kv) * a.H * a.D +
        hp * 8);
    uint16_t* dst;
    if constexpr (Paged) {
      const int64_t r = paged_row(a.table, a.tstride, a.n_pages, a.psh, a.H, b, h, pos);
      if (r < 0) continue;
      dst = (kv ? a.v_cache : a.k_cache) + r * a.D + piece * 8;
    } else {
      dst = (kv ? a.v_cache : a.k_cache) +
            ((static_cast<int64_t>(b) * a.H + h) * a.L_max + pos) * a.D + piece * 8;
    }
    *reinterpret_cast<u16x8*>(dst) = val;
  }
}

struct KvAppend8Args {
  const uint16_t* qkv;   // [B, T, 3, H, D], token row stride ld
  uint8_t* k_cache;      // [B, H, L_max, D] e4m3fn
  uint8_t* v_cache;
  float* k_scale;        // [B, H, L_max]
  float* v_scale;
  const int* length;
  int64_t ld;
  int B, T, H, L_max;
  const int* table;      // Paged, as in KvAppendArgs
  int64_t tstride;
  int n_pages, psh;
};

// a row (b, t, k|v, h) of D bf16 per group of D / 8 lanes; uniform trip count over the grid, so
// every lane of a group is active in the shuffles
template <int D, bool PerSeq, bool Paged>
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(KvAppend8Args a) {
  constexpr int LG = D / 8;                                 // lanes per row
  [[maybe_unused]] const int len0 = PerSeq ? 0 : *a.length;
  const int64_t rows = static_cast<int64_t>(a.B) * a.T * 2 * a.H;
  const int64_t step = static_cast<int64_t>(gridDim.x) * blockDim.x / LG;
  const int piece = threadIdx.x % LG;
  const int64_t first = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) / LG;
  for (int64_t r0 = 0; r0 < rows; r0 += step) {
    const int64_t r = r0 + first;
    const bool live = r < rows;
    const int64_t rr = live ? r : 0;
    const int64_t tok = rr / (2 * a.H);
    const int kh = static_cast<int>(rr - tok * 2 * a.H);    // (k|v, h)
    const int kv = kh / a.H, h = kh - kv * a.H;
    const int b = static_cast<int>(tok / a.T), t = static_cast<int>(tok - (int64_t)b * a.T);
    const u16x8 x = *reinterpret_cast<const u16x8*>(
        a.qkv + tok * a.ld + static_cast<int64_t>(1 + kv) * a.H * D + h * D + piece * 8);
    float f[8], amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f[j] = bf16_to_f32(x[j]);
      amax = __builtin_fmaxf(amax, __builtin_fabsf(f[j]));
    }
#pragma unroll
    for (int off = 1; off < LG; off <<= 1) amax = __builtin_fmaxf(amax, __shfl_xor(amax, off, 64));
    float inv, scale;
    row_scale(amax, inv, scale);
    int len;
    if constexpr (PerSeq) len = a.length[b];                // b < B also for a dead lane (rr = 0)
    else len = len0;
    const int64_t pos = static_cast<int64_t>(len) + t;
    if (!live || len < 0 || pos >= a.L_max) continue;       // device-side guard: never past the cache
    int64_t dst;
    if constexpr (Paged) {
      dst = paged_row(a.table, a.tstride, a.n_pages, a.psh, a.H, b, h, pos);
      if (dst < 0) continue;                                // an unmapped page: dropped
    } else {
      dst = (static_cast<int64_t>(b) * a.H + h) * a.L_max + pos;
    }
    const u32x2 code{f32x4_to_e4m3(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv),
                     f32x4_to_e4m3(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv)};
    *reinterpret_cast<u32x2*>((kv ? a.v_cache : a.k_cache) + dst * D + piece * 8) = code;
    if (piece == 0) (kv ? a.v_scale : a.k_scale)[dst] = scale;
  }
}

struct DecodeArgs {
  const uint16_t* qkv;   // [B, 1, 3, H, D], batch row stride ld
  uint8_t* k_cache;      // [B, H, L_max, D] bf16 or e4m3fn
  uint8_t* v_cache;
  float* k_scale;        // [B, H, L_max]; null for the bf16 cache
  float* v_scale;
  const int* length;
  float* ws;             // [B, H, n_chunks, D + 2]: m, l, o[D]
  uint16_t* out;         // [B, 1, H, D], batch row stride ldo
  int64_t ld, ldo;
  int B, H, L_max, chunk, n_chunks, fused;
  float scale_log2;
  // Paged (after the contiguous forms' fields, whose offsets stay): k_cache / v_cache / k_scale /
  // v_scale are the pools [n_pages, H, P, D] / [n_pages, H, P]
  const int* table;      // [B, tstride]
  int64_t tstride;
  int n_pages, psh;      // P = 1 << psh
};

constexpr int kDecChunkPages = 64;     // table entries of one chunk: one per lane of a wave

// the split kernel's LDS copy of its chunk's table entries (-1 = unmapped); no LDS when !Paged
template <bool Paged>
__device__ __forceinline__ int* chunk_pages() {
  if constexpr (Paged) {
    __shared__ int pages[kDecChunkPages];
    return pages;
  } else {
    return nullptr;
  }
}

// keys the step attends (and whether the new token has a cache slot): uniform, from device
// memory. PerSeq: row b's own length; a negative one is an empty slot, 0 keys, len stays < 0
template <bool PerSeq>
__device__ __forceinline__ int decode_keys(const DecodeArgs& a, int b, int& len, bool& room) {
  if constexpr (PerSeq) {
    len = a.length[b];
    room = len < a.L_max;
    if (len < 0) return 0;
  } else {
    len = *a.length;
    if (len < 0) len = 0;
    room = len < a.L_max;
  }
  return room ? len + 1 : a.L_max;
}

// What differs between the cache formats: a lane's 16-byte fragment of a row (kCols columns of
// Elem) and its widening to floats, and whether rows carry a scale.
struct KvBf16 {
  using Elem = uint16_t;
  using Frag = u16x8;
  static constexpr int kCols = 8;
  static constexpr bool kScaled = false;
  static __device__ __forceinline__ void widen(const Frag& r, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf16_to_f32(r[j]);
  }
};
struct KvE4m3 {
  using Elem = uint8_t;
  using Frag = u32x4;
  static constexpr int kCols = 16;
  static constexpr bool kScaled = true;
  static __device__ __forceinline__ void widen(const Frag& r, float (&v)[16]) {
    e4m3x16_to_f32(r, v);
  }
};

// 16 bf16 columns of a row held by LPK lanes -> the row's codes of these columns and its scale
template <int LPK>
__device__ __forceinline__ void quant_row16(const uint16_t* p, u32x4& code, float& scale) {
  const u16x8 x0 = *reinterpret_cast<const u16x8*>(p);
  const u16x8 x1 = *reinterpret_cast<const u16x8*>(p + 8);
  float f[16], amax = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f[j] = bf16_to_f32(x0[j]);
    f[8 + j] = bf16_to_f32(x1[j]);
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) amax = __builtin_fmaxf(amax, __builtin_fabsf(f[j]));
#pragma unroll
  for (int off = 1; off < LPK; off <<= 1) amax = __builtin_fmaxf(amax, __shfl_xor(amax, off, 64));
  float inv;
  row_scale(amax, inv, scale);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    code[i] = f32x4_to_e4m3(f[4 * i] * inv, f[4 * i + 1] * inv, f[4 * i + 2] * inv,
                            f[4 * i + 3] * inv);
}

template <int D, typename Fmt, bool PerSeq, bool Paged>
__global__ __launch_bounds__(kDecThreads) void attn_decode_split_kernel(DecodeArgs a) {
  using Elem = typename Fmt::Elem;
  using Frag = typename Fmt::Frag;
  constexpr int C = Fmt::kCols;              // columns per lane (16 B)
  constexpr int LPK = D / C;                 // lanes per key
  constexpr int NS = kDecThreads / LPK;      // key slots per workgroup
  constexpr int U = kDecUnroll;
  __shared__ float red[kDecThreads / kWave][D + 2];

  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  int len;
  bool room;
  const int L = decode_keys<PerSeq>(a, b, len, room);
  const int k0 = c * a.chunk;
  if (k0 >= L) return;                       // dead chunk (every chunk of an empty slot): no K / V
                                             // read, no partial written
  const int k1 = min(k0 + a.chunk, L);
  const int tid = threadIdx.x, sub = tid % LPK, slot = tid / LPK;
  // position whose K / V come from qkv (and are stored to the cache here); -1: none
  const int newpos = (a.fused && room) ? len : -1;

  // Paged: the chunk's table entries, once per workgroup. Every wave loads them (one entry per
  // lane: a chunk starts on a page edge and holds <= 64 pages), entries outside the pool become
  // -1, the ballot gives the first mapped page: masked and unmapped keys re-read its row 0,
  // logical position ksafe < k1 (a cached row, or the token: `fresh` below). Wave 0 keeps the
  // entries in LDS for the per-key look-ups.
  [[maybe_unused]] int* pages = chunk_pages<Paged>();
  [[maybe_unused]] int ksafe = 0, pgsafe = 0;
  if constexpr (Paged) {
    const int ln = tid & (kWave - 1);
    const int n_ent = (k1 - k0 + (1 << a.psh) - 1) >> a.psh;
    int e = -1;
    if (ln < n_ent) e = a.table[b * a.tstride + (k0 >> a.psh) + ln];
    if (e < 0 || e >= a.n_pages) e = -1;
    const unsigned long long mapped = __ballot(e >= 0);
    if (mapped == 0) {                       // no mapped page: the partial of no keys
      if (tid < D) {
        float* p = a.ws + ((static_cast<int64_t>(b) * a.H + h) * a.n_chunks + c) * (D + 2);
        p[2 + tid] = 0.f;
        if (tid == 0) {
          p[0] = kDecNegBig;
          p[1] = 0.f;
        }
      }
      return;
    }
    const int first = __builtin_ctzll(mapped);
    ksafe = k0 + (first << a.psh);
    pgsafe = __shfl(e, first, 64);
    if (tid < kWave) pages[tid] = e;
    __syncthreads();
  }

  // The compiler's schedule and register allocation of the whole kernel follow the statement
  // order of this prologue and the way its address sums associate. Where the two formats differ
  // below in nothing else, each keeps the order its measured kernel was built from
  // (docs/PERFORMANCE.md, "One core for the bf16 and FP8 decode kernels").
  const uint16_t* row = a.qkv + static_cast<int64_t>(b) * a.ld + h * D + sub * C;
  // bf16: the token's K / V are read where the loop meets them, and copied to the cache there
  [[maybe_unused]] const uint16_t *nkp = nullptr, *nvp = nullptr;
  if constexpr (!Fmt::kScaled) {
    nkp = row + a.H * D;
    nvp = row + 2 * a.H * D;
  }
  float q[C];                                // the lane's C columns of the query
  if constexpr (C == 8) {
    KvBf16::widen(*reinterpret_cast<const u16x8*>(row), q);
  } else {
    const u16x8 q0 = *reinterpret_cast<const u16x8*>(row);
    const u16x8 q1 = *reinterpret_cast<const u16x8*>(row + 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      q[j] = bf16_to_f32(q0[j]);
      q[8 + j] = bf16_to_f32(q1[j]);
    }
  }
  const int64_t rows = (static_cast<int64_t>(b) * a.H + h) * a.L_max;
  // the lane's columns of row 0 of (b, h): cache + rows * D + sub * C
  Elem *kc = reinterpret_cast<Elem*>(a.k_cache), *vc = reinterpret_cast<Elem*>(a.v_cache);
  if constexpr (Paged) {                     // pool row 0; `rows` is not used
    kc += sub * C;
    vc += sub * C;
  } else if constexpr (Fmt::kScaled) {
    kc = kc + rows * D + sub * C;
    vc = vc + rows * D + sub * C;
  } else {
    kc += rows * D + sub * C;
    vc += rows * D + sub * C;
  }

  // FP8: the append, by the chunk owning `length` (workgroup-uniform): every slot holds the
  // token's codes and scales, slot 0 stores them
  [[maybe_unused]] float *ksc = nullptr, *vsc = nullptr;
  [[maybe_unused]] Frag nk{}, nv{};
  [[maybe_unused]] float nks = 1.f, nvs = 1.f;
  if constexpr (Fmt::kScaled) {
    if constexpr (Paged) {
      ksc = a.k_scale;
      vsc = a.v_scale;
    } else {
      ksc = a.k_scale + rows;
      vsc = a.v_scale + rows;
    }
    if (newpos >= k0 && newpos < k1) {
      quant_row16<LPK>(row + a.H * D, nk, nks);
      quant_row16<LPK>(row + 2 * a.H * D, nv, nvs);
      if constexpr (Paged) {                 // through the table; dropped on an unmapped page
        const int pg = pages[(newpos - k0) >> a.psh];
        const int64_t nr = pool_row(pg, a.H, h, a.psh, newpos);
        if (slot == 0 && pg >= 0) {
          *reinterpret_cast<Frag*>(kc + nr * D) = nk;
          *reinterpret_cast<Frag*>(vc + nr * D) = nv;
          if (sub == 0) {
            ksc[nr] = nks;
            vsc[nr] = nvs;
          }
        }
      } else if (slot == 0) {
        *reinterpret_cast<Frag*>(kc + static_cast<int64_t>(newpos) * D) = nk;
        *reinterpret_cast<Frag*>(vc + static_cast<int64_t>(newpos) * D) = nv;
        if (sub == 0) {
          ksc[newpos] = nks;
          vsc[newpos] = nvs;
        }
      }
    }
  }

  float m = kDecNegBig, l = 0.f, o[C];
#pragma unroll
  for (int j = 0; j < C; ++j) o[j] = 0.f;

  for (int it = k0; it < k1; it += NS * U) {       // uniform trip count over the workgroup
    Frag kr[U], vr[U];
    [[maybe_unused]] float ks[U], vs[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = it + u * NS + slot;
      ok[u] = key < k1;
      int kk = ok[u] ? key : k1 - 1;               // masked slots re-read a live row
      [[maybe_unused]] int64_t r = 0;              // Paged: the pool row holding key kk
      if constexpr (Paged) {
        const int pg = pages[(kk - k0) >> a.psh];
        const bool mapped = pg >= 0;               // a key on an unmapped page is masked too
        ok[u] = ok[u] && mapped;
        kk = mapped ? kk : ksafe;
        r = pool_row(mapped ? pg : pgsafe, a.H, h, a.psh, kk);
      }
      const bool fresh = kk == newpos;
      Elem* kp = kc + (Paged ? r : static_cast<int64_t>(kk)) * D;
      Elem* vp = vc + (Paged ? r : static_cast<int64_t>(kk)) * D;
      if constexpr (Fmt::kScaled) {
        // row `newpos` is taken from the registers, never from what the loads below return for it
        // (slot 0's stores may or may not have landed): the loads stay in bounds, kk < L <= L_max
        const Frag kl = *reinterpret_cast<const Frag*>(kp);
        const Frag vl = *reinterpret_cast<const Frag*>(vp);
        const float ksl = Paged ? ksc[r] : ksc[kk], vsl = Paged ? vsc[r] : vsc[kk];
        kr[u] = fresh ? nk : kl;
        vr[u] = fresh ? nv : vl;
        ks[u] = fresh ? nks : ksl;
        vs[u] = fresh ? nvs : vsl;
      } else {
        kr[u] = *reinterpret_cast<const Frag*>(fresh ? nkp : kp);
        vr[u] = *reinterpret_cast<const Frag*>(fresh ? nvp : vp);
        if (fresh && ok[u]) {                      // the append, by the chunk owning `length`
          *reinterpret_cast<Frag*>(kp) = kr[u];
          *reinterpret_cast<Frag*>(vp) = vr[u];
        }
      }
    }
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[C];
      Fmt::widen(kr[u], kf);
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < C; ++j) d = __builtin_fmaf(q[j], kf[j], d);
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) d += __shfl_xor(d, off, 64);
      if constexpr (Fmt::kScaled) d = d * ks[u];
      s[u] = ok[u] ? d * a.scale_log2 : kDecNegBig;
    }
    float mn = m;
#pragma unroll
    for (int u = 0; u < U; ++u) mn = fmaxf(mn, s[u]);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    l *= alpha;
#pragma unroll
    for (int j = 0; j < C; ++j) o[j] *= alpha;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float p = ok[u] ? __builtin_amdgcn_exp2f(s[u] - mn) : 0.f;
      float vf[C];
      Fmt::widen(vr[u], vf);
      l += p;
      if constexpr (Fmt::kScaled) p = p * vs[u];
#pragma unroll
      for (int j = 0; j < C; ++j) o[j] = __builtin_fmaf(p, vf[j], o[j]);
    }
    m = mn;
  }

  // merge the slots of a wave (lanes sub, sub + LPK, ...): butterfly, same value on both sides
#pragma unroll
  for (int off = LPK; off < kWave; off <<= 1) {
    const float m2 = __shfl_xor(m, off, 64), l2 = __shfl_xor(l, off, 64);
    const float mn = fmaxf(m, m2);
    const float f1 = __builtin_amdgcn_exp2f(m - mn), f2 = __builtin_amdgcn_exp2f(m2 - mn);
    // the partner computes l2' * f1' + l' * f2' with the roles swapped: order the two products
    // by lane so both lanes round identically
    const bool lo = (tid & off) == 0;
    const float la = lo ? l * f1 : l2 * f2, lb = lo ? l2 * f2 : l * f1;
    l = la + lb;
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const float o2 = __shfl_xor(o[j], off, 64);
      const float oa = lo ? o[j] * f1 : o2 * f2, ob = lo ? o2 * f2 : o[j] * f1;
      o[j] = oa + ob;
    }
    m = mn;
  }
  const int lane = tid & (kWave - 1), w = tid / kWave;
  if (lane < LPK) {
#pragma unroll
    for (int j = 0; j < C; ++j) red[w][sub * C + j] = o[j];
    if (sub == 0) {
      red[w][D] = m;
      red[w][D + 1] = l;
    }
  }
  __syncthreads();
  if (tid < D) {                                   // the 4 waves, in wave order
    float mw = red[0][D];
#pragma unroll
    for (int i = 1; i < kDecThreads / kWave; ++i) mw = fmaxf(mw, red[i][D]);
    float lw = 0.f, ow = 0.f;
#pragma unroll
    for (int i = 0; i < kDecThreads / kWave; ++i) {
      const float f = __builtin_amdgcn_exp2f(red[i][D] - mw);
      lw = __builtin_fmaf(red[i][D + 1], f, lw);
      ow = __builtin_fmaf(red[i][tid], f, ow);
    }
    float* p = a.ws + ((static_cast<int64_t>(b) * a.H + h) * a.n_chunks + c) * (D + 2);
    p[2 + tid] = ow;
    if (tid == 0) {
      p[0] = mw;
      p[1] = lw;
    }
  }
}

// grid (H, B), D threads: thread d owns output column d of head h
template <int D, bool PerSeq>
__global__ __launch_bounds__(D) void attn_decode_combine_kernel(DecodeArgs a) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  int len;
  bool room;
  const int L = decode_keys<PerSeq>(a, b, len, room);
  if constexpr (PerSeq) {
    if (len < 0) {                                   // an empty slot has no partials: zeros
      a.out[static_cast<int64_t>(b) * a.ldo + h * D + d] = 0;
      return;
    }
  }
  const int live = min((L + a.chunk - 1) / a.chunk, a.n_chunks);
  const float* p = a.ws + (static_cast<int64_t>(b) * a.H + h) * a.n_chunks * (D + 2);
  float mx = kDecNegBig;
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
  a.out[static_cast<int64_t>(b) * a.ldo + h * D + d] = f32_to_bf16(acc / lsum);
}

bool mis(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

// what all four entry points ask of qkv, the cache geometry and `length`
bool qkv_cache_ok(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache,
                  const void* length, int H, int D, int L_max) {
  if (D != 64 && D != 128) return false;
  if (L_max <= 0 || ld % 8 || ld < 3 * H * D || !length) return false;
  return !(mis(qkv, 16) || mis(k_cache, 16) || mis(v_cache, 16));
}

// the per-sequence `length`: int32[B], read as length[b]
bool seq_length_ok(const void* length) { return length && !mis(length, 4); }

// the FP8 cache's scale planes
bool scales_ok(const void* k_scale, const void* v_scale) {
  return k_scale && v_scale && !mis(k_scale, 4) && !mis(v_scale, 4);
}

// the block table of a paged launch (all zero for the contiguous forms)
struct PageTable {
  const void* table;     // int32[B, stride]
  int64_t stride;
  int n_pages, P;
};

// what the paged entry points ask of the table and the page size: P a power of two in [16, 256],
// a row of the table covers L_max, and (decode: chunk > 0) a chunk is 1 .. 64 whole pages
bool paged_ok(const PageTable& t, int L_max, int chunk, int& psh) {
  if (!t.table || mis(t.table, 4) || t.n_pages <= 0) return false;
  if (t.P < 16 || t.P > 256 || (t.P & (t.P - 1))) return false;
  if (t.stride < (static_cast<int64_t>(L_max) + t.P - 1) / t.P) return false;
  if (chunk > 0 && (chunk % t.P || chunk / t.P > kDecChunkPages)) return false;
  psh = __builtin_ctz(t.P);
  return true;
}

// validation and the split + combine launches of the decode entry points
template <typename Fmt, bool PerSeq, bool Paged = false>
int decode_launch(const void* qkv, int64_t ld, void* k_cache, void* v_cache, void* k_scale,
                  void* v_scale, const void* length, void* ws, void* out, int64_t ldo, int B,
                  int H, int D, int L_max, int len_bound, int chunk, int fused, float scale,
                  hipStream_t stream, const PageTable& pt = {}) {
  if (B <= 0 || H <= 0) return hipSuccess;
  if (!qkv_cache_ok(qkv, ld, k_cache, v_cache, length, H, D, L_max)) return hipErrorInvalidValue;
  if (PerSeq && !seq_length_ok(length)) return hipErrorInvalidValue;
  if (chunk <= 0 || len_bound <= 0 || !ws || ldo < H * D) return hipErrorInvalidValue;
  if (!k_cache || !v_cache || !out) return hipErrorInvalidValue;
  if (Fmt::kScaled && !scales_ok(k_scale, v_scale)) return hipErrorInvalidValue;
  if (H > 65535 || B > 65535) return hipErrorInvalidValue;
  int psh = 0;
  if (Paged && !paged_ok(pt, L_max, chunk, psh)) return hipErrorInvalidValue;
  if (len_bound > L_max) len_bound = L_max;
  const int n_chunks = (len_bound + chunk - 1) / chunk;
  DecodeArgs a{static_cast<const uint16_t*>(qkv), static_cast<uint8_t*>(k_cache),
               static_cast<uint8_t*>(v_cache), static_cast<float*>(k_scale),
               static_cast<float*>(v_scale), static_cast<const int*>(length),
               static_cast<float*>(ws), static_cast<uint16_t*>(out), ld, ldo, B, H, L_max, chunk,
               n_chunks, fused ? 1 : 0, scale * 1.4426950408889634f,
               static_cast<const int*>(pt.table), pt.stride, pt.n_pages, psh};
  const dim3 gs(n_chunks, H, B), gc(H, B);
  if (D == 64) {
    hipLaunchKernelGGL((attn_decode_split_kernel<64, Fmt, PerSeq, Paged>), gs, dim3(kDecThreads),
                       0, stream, a);
    hipLaunchKernelGGL((attn_decode_combine_kernel<64, PerSeq>), gc, dim3(64), 0, stream, a);
  } else {
    hipLaunchKernelGGL((attn_decode_split_kernel<128, Fmt, PerSeq, Paged>), gs, dim3(kDecThreads),
                       0, stream, a);
    hipLaunchKernelGGL((attn_decode_combine_kernel<128, PerSeq>), gc, dim3(128), 0, stream, a);
  }
  return hipGetLastError();
}

// validation and the launch of the bf16 append entry points
template <bool PerSeq, bool Paged = false>
int append_launch(const void* qkv, int64_t ld, void* k_cache, void* v_cache, const void* length,
                  int B, int T, int H, int D, int L_max, hipStream_t stream,
                  const PageTable& pt = {}) {
  if (B <= 0 || T <= 0 || H <= 0) return hipSuccess;
  if (!qkv_cache_ok(qkv, ld, k_cache, v_cache, length, H, D, L_max)) return hipErrorInvalidValue;
  if (PerSeq && !seq_length_ok(length)) return hipErrorInvalidValue;
  int psh = 0;
  if (Paged && !paged_ok(pt, L_max, 0, psh)) return hipErrorInvalidValue;
  KvAppendArgs a{static_cast<const uint16_t*>(qkv), static_cast<uint16_t*>(k_cache),
                 static_cast<uint16_t*>(v_cache), static_cast<const int*>(length), ld, B, T, H, D,
                 L_max, static_cast<const int*>(pt.table), pt.stride, pt.n_pages, psh};
  const int64_t vecs = static_cast<int64_t>(B) * T * 2 * H * (D / 8);
  hipLaunchKernelGGL((kv_append_kernel<PerSeq, Paged>), dim3(stream_grid(vecs, 256)), dim3(256),
                     0, stream, a);
  return hipGetLastError();
}

// the same for the FP8 append entry points
template <bool PerSeq, bool Paged = false>
int append_fp8_launch(const void* qkv, int64_t ld, void* k_cache, void* v_cache, void* k_scale,
                      void* v_scale, const void* length, int B, int T, int H, int D, int L_max,
                      hipStream_t stream, const PageTable& pt = {}) {
  if (B <= 0 || T <= 0 || H <= 0) return hipSuccess;
  if (!qkv_cache_ok(qkv, ld, k_cache, v_cache, length, H, D, L_max)) return hipErrorInvalidValue;
  if (PerSeq && !seq_length_ok(length)) return hipErrorInvalidValue;
  if (!k_cache || !v_cache || !scales_ok(k_scale, v_scale)) return hipErrorInvalidValue;
  int psh = 0;
  if (Paged && !paged_ok(pt, L_max, 0, psh)) return hipErrorInvalidValue;
  KvAppend8Args a{static_cast<const uint16_t*>(qkv), static_cast<uint8_t*>(k_cache),
                  static_cast<uint8_t*>(v_cache), static_cast<float*>(k_scale),
                  static_cast<float*>(v_scale), static_cast<const int*>(length), ld, B, T, H,
                  L_max, static_cast<const int*>(pt.table), pt.stride, pt.n_pages, psh};
  const int64_t lanes = static_cast<int64_t>(B) * T * 2 * H * (D / 8);
  const dim3 grid(stream_grid(lanes, 256));
  if (D == 64)
    hipLaunchKernelGGL((kv_append_fp8_kernel<64, PerSeq, Paged>), grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL((kv_append_fp8_kernel<128, PerSeq, Paged>), grid, dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

}  // namespace dlbb

using namespace dlbb;

// qkv: [B, T, 3, H, D] bf16 (token row stride ld elements); k_cache / v_cache: [B, H, L_max, D]
// bf16 contiguous; length: device int32. Rows K / V of every token go to cache positions
// [*length, *length + T); positions >= L_max are dropped on the device.
DLBB_API int dlbb_kv_append(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                            const void* length, int B, int T, int H, int D, int L_max,
                            hipStream_t stream) {
  return append_launch<false>(qkv, ld, k_cache, v_cache, length, B, T, H, D, L_max, stream);
}

// Per-sequence lengths: length is device int32[B]; row b's tokens go to positions [length[b],
// length[b] + T), nothing is written for a row with length[b] < 0.
DLBB_API int dlbb_kv_append_seq(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                const void* length, int B, int T, int H, int D, int L_max,
                                hipStream_t stream) {
  return append_launch<true>(qkv, ld, k_cache, v_cache, length, B, T, H, D, L_max, stream);
}

// The same for the FP8 cache: k_cache / v_cache [B, H, L_max, D] e4m3fn contiguous, k_scale /
// v_scale [B, H, L_max] fp32 contiguous. Rows K / V of every token are quantised to cache
// positions [*length, *length + T); positions >= L_max (and every position when *length < 0) are
// dropped on the device.
DLBB_API int dlbb_kv_append_fp8(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                void* k_scale, void* v_scale, const void* length, int B, int T,
                                int H, int D, int L_max, hipStream_t stream) {
  return append_fp8_launch<false>(qkv, ld, k_cache, v_cache, k_scale, v_scale, length, B, T, H, D,
                                  L_max, stream);
}

// The FP8 append with per-sequence lengths (dlbb_kv_append_seq's contract).
DLBB_API int dlbb_kv_append_fp8_seq(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                    void* k_scale, void* v_scale, const void* length, int B,
                                    int T, int H, int D, int L_max, hipStream_t stream) {
  return append_fp8_launch<true>(qkv, ld, k_cache, v_cache, k_scale, v_scale, length, B, T, H, D,
                                 L_max, stream);
}

// One decode step of attention: qkv [B, 1, 3, H, D] (batch row stride ld), the bf16 cache as
// above, out [B, 1, H, D] bf16 (batch row stride ldo). Attends over *length + 1 keys; with
// fused != 0 the new token's K / V are taken from qkv and stored at position *length by the same
// launch, else the caller has appended them already. ws: fp32 [B, H, n_chunks, D + 2], n_chunks =
// ceil(min(len_bound, L_max) / chunk); len_bound is the host's upper bound of *length + 1.
DLBB_API int dlbb_attn_decode(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                              const void* length, void* ws, void* out, int64_t ldo, int B, int H,
                              int D, int L_max, int len_bound, int chunk, int fused, float scale,
                              hipStream_t stream) {
  return decode_launch<KvBf16, false>(qkv, ld, k_cache, v_cache, nullptr, nullptr, length, ws, out, ldo,
                               B, H, D, L_max, len_bound, chunk, fused, scale, stream);
}

// The same over the FP8 cache: with fused != 0 the new token's K / V are quantised from qkv,
// stored at position *length and attended to in their quantised form.
DLBB_API int dlbb_attn_decode_fp8(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                  void* k_scale, void* v_scale, const void* length, void* ws,
                                  void* out, int64_t ldo, int B, int H, int D, int L_max,
                                  int len_bound, int chunk, int fused, float scale,
                                  hipStream_t stream) {
  return decode_launch<KvE4m3, false>(qkv, ld, k_cache, v_cache, k_scale, v_scale, length, ws, out, ldo,
                               B, H, D, L_max, len_bound, chunk, fused, scale, stream);
}

// The decode step with per-sequence lengths: length is device int32[B], row b attends over
// length[b] + 1 keys (L_max keys and no store when length[b] >= L_max); a row with length[b] < 0
// is an empty slot: nothing read or stored, its output row is zeros. len_bound is the host's upper
// bound of max_b length[b] + 1.
DLBB_API int dlbb_attn_decode_seq(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                  const void* length, void* ws, void* out, int64_t ldo, int B,
                                  int H, int D, int L_max, int len_bound, int chunk, int fused,
                                  float scale, hipStream_t stream) {
  return decode_launch<KvBf16, true>(qkv, ld, k_cache, v_cache, nullptr, nullptr, length, ws, out,
                                     ldo, B, H, D, L_max, len_bound, chunk, fused, scale, stream);
}

// The same over the FP8 cache.
DLBB_API int dlbb_attn_decode_fp8_seq(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                      void* k_scale, void* v_scale, const void* length, void* ws,
                                      void* out, int64_t ldo, int B, int H, int D, int L_max,
                                      int len_bound, int chunk, int fused, float scale,
                                      hipStream_t stream) {
  return decode_launch<KvE4m3, true>(qkv, ld, k_cache, v_cache, k_scale, v_scale, length, ws, out,
                                     ldo, B, H, D, L_max, len_bound, chunk, fused, scale, stream);
}

// The paged forms (file header): k_pool / v_pool [n_pages, H, P, D] (FP8: k_scale / v_scale
// [n_pages, H, P]), block_table device int32[B, table_stride] with table_stride >= ceil(L_max / P),
// length device int32[B] under the *_seq rules, L_max the logical cap. P must be a power of two in
// [16, 256]; the decode forms also need chunk to be 1 .. 64 whole pages. Anything else, a null or
// misaligned table or n_pages <= 0 returns hipErrorInvalidValue before any launch. A position
// whose table entry lies outside [0, n_pages) is never stored to and never attended.
DLBB_API int dlbb_kv_append_paged(const void* qkv, int64_t ld, void* k_pool, void* v_pool,
                                  const void* length, const void* block_table,
                                  int64_t table_stride, int n_pages, int P, int B, int T, int H,
                                  int D, int L_max, hipStream_t stream) {
  return append_launch<true, true>(qkv, ld, k_pool, v_pool, length, B, T, H, D, L_max, stream,
                                   PageTable{block_table, table_stride, n_pages, P});
}

DLBB_API int dlbb_kv_append_fp8_paged(const void* qkv, int64_t ld, void* k_pool, void* v_pool,
                                      void* k_scale, void* v_scale, const void* length,
                                      const void* block_table, int64_t table_stride, int n_pages,
                                      int P, int B, int T, int H, int D, int L_max,
                                      hipStream_t stream) {
  return append_fp8_launch<true, true>(qkv, ld, k_pool, v_pool, k_scale, v_scale, length, B, T, H,
                                       D, L_max, stream,
                                       PageTable{block_table, table_stride, n_pages, P});
}

DLBB_API int dlbb_attn_decode_paged(const void* qkv, int64_t ld, void* k_pool, void* v_pool,
                                    const void* length, const void* block_table,
                                    int64_t table_stride, int n_pages, int P, void* ws, void* out,
                                    int64_t ldo, int B, int H, int D, int L_max, int len_bound,
                                    int chunk, int fused, float scale, hipStream_t stream) {
  return decode_launch<KvBf16, true, true>(qkv, ld, k_pool, v_pool, nullptr, nullptr, length, ws,
                                           out, ldo, B, H, D, L_max, len_bound, chunk, fused,
                                           scale, stream,
                                           PageTable{block_table, table_stride, n_pages, P});
}

DLBB_API int dlbb_attn_decode_fp8_paged(const void* qkv, int64_t ld, void* k_pool, void* v_pool,
                                        void* k_scale, void* v_scale, const void* length,
                                        const void* block_table, int64_t table_stride,
                                        int n_pages, int P, void* ws, void* out, int64_t ldo,
                                        int B, int H, int D, int L_max, int len_bound, int chunk,
                                        int fused, float scale, hipStream_t stream) {
  return decode_launch<KvE4m3, true, true>(qkv, ld, k_pool, v_pool, k_scale, v_scale, length, ws,
                                           out, ldo, B, H, D, L_max, len_bound, chunk, fused,
                                           scale, stream,
                                           PageTable{block_table, table_stride, n_pages, P});
}
