// Chunked prefill: causal attention of a block of T new tokens over a KV cache, gfx950 (MI355X,
// CDNA4), bf16 or FP8 (e4m3fn) cache, head dim 64 / 128.
//
// Contract. qkv is the chunk's fused activation [B, T, 3, H, D] bf16 (token row stride ld); its
// K / V rows were appended to the cache at [len_b, len_b + T) by dlbb_kv_append* BEFORE this
// launch and `length` has not been advanced: len_b is the word the append read (*length, or
// length[b] for the per-sequence and paged forms), read here from device memory too. Query i of
// row b attends cache positions 0 .. len_b + i (the causal mask is bottom-right aligned); EVERY
// key and value comes from the cache, only Q from qkv. Output [B, T, H * D] bf16 (row stride
// ldo), heads interleaved as attn_fwd writes it. No LSE, no workspace, no atomics: bit-identical
// from run to run. len_b < 0 is an empty slot: zero rows out, nothing loaded. Positions at or
// past kend = min(len_b + T, L_max) are never loaded (stale rows may hold NaN bit patterns, and
// 0 * NaN is NaN in the PV product): a tile row past kend is redirected to position kend - 1 and
// its score masked.
//
// One kernel template <D, PerSeq, Paged, Fp8> on attn_fwd_kernel's tile geometry (attn_tile.h):
// a workgroup of 4 waves takes 128 queries of one (b, h), a lane owns one query (S^T = K Q^T on
// v_mfma_f32_32x32x16_bf16), K / V tiles are 8-KiB images (64 keys at D = 64, 32 at D = 128)
// staged by LDS-DMA (bf16 cache), double buffered, read back with ds_read_b128 (K rows) and
// ds_read_b64_tr_b16 (V, transposed) under the same swizzles; the softmax keeps the deferred
// running max. What differs from the forward:
//   * Sources. A key tile is KB consecutive cache rows of 2 D bytes: a lane's DMA source is
//     row * D in one [L_max, D] run of (b, h), not row * ld + section of qkv.
//   * Key loop. nt = ceil(min(len_b + min(q0 + 128, T), L_max) / KB) from the device length; the
//     grid (ceil(T / 128), H, B) depends on the shapes alone. len_b is arbitrary, so the diagonal
//     is not tile-aligned: a lane's last visible key is lim = min(len_b + q, kend - 1) and its
//     threshold inside a tile lim - k0 - 4 hi. Only tiles whose last key lies beyond the WAVE's
//     first query's limit are masked; the prefix tiles run the unmasked path.
//   * "No key" is finite (-1e30, as the decode kernels' kDecNegBig) and the running max starts
//     at half of it (scaled), above every masked score and below every real one: a lane all of
//     whose keys in a tile are masked gets p = exp2(-huge) = 0 there and keeps its max, and one
//     with no visible key at all ends with l = 0 and writes zeros; no inf - inf anywhere.
//   * Paged. A 16-key group of a tile lies in one page (P >= 16, tiles start on multiples of
//     KB), so a tile has KB / 16 <= 4 table entries. They are wave-uniform loads (the same word
//     for every lane: scalar registers), made by every wave when it stages the tile, so all four
//     waves hold the same <= 4 validity bits without a round trip through LDS. An entry outside
//     [0, n_pages) never becomes an address: the rows of its group are loaded from the first
//     mapped live group of the same tile and the group's scores are masked; a tile with no
//     mapped group is neither loaded nor computed (the arithmetic of masking it whole: p = 0,
//     max kept). A tile with every page mapped, the common case, takes exactly the contiguous
//     kernel's path, so with equal contents the output has the bits of the per-sequence launch.
//   * Work order. Query blocks run heaviest (last) first. No causal pairing (attn_fwd pairs
//     block i with nqb - 1 - i): a block's work is len_b + 128 (i + 1) keys, so pairing levels
//     only the chunk's own share and the imbalance it removes shrinks as (len_b + T) /
//     (len_b + 128) -> 1 when the prefix dominates, while it halves the number of workgroups —
//     and a short chunk over a long prefix already under-fills 256 CUs with ceil(T / 128) H B of
//     them. len_b is also a device value, so the host could not choose per launch. The block
//     order is the XCD-aware one (head_block): the query blocks of a head share one L2 and read
//     the head's prefix from HBM once.
//
// FP8 cache (template parameter Fp8; dlbb_attn_prefill_fp8{,_seq,_paged}). k_cache / v_cache hold
// e4m3fn codes [B, H, L_max, D] (pools [n_pages, H, P, D]) and k_scale / v_scale one fp32 scale
// per row [B, H, L_max] ([n_pages, H, P]), as dlbb_kv_append_fp8* wrote them: a row is
// float(code) * scale. Every rule above holds; the chunk attends to its own rows in their
// quantised form. The bf16 instantiations compile to the instructions they had before.
//   * Staging. An FP8 tile cannot go global -> LDS by DMA and still be read as bf16 MFMA
//     operands, so it goes through registers: right after the barrier that frees the other
//     buffer each thread issues one 16-byte global load of K codes and one of V codes of tile
//     kt + 1 (KB * D / 256 = 16 codes per operand; the threads of a row's first two runs also
//     load its k- / v-scale), the loads fly while tile kt is computed, and before the next barrier
//     the thread widens them and writes the SAME swizzled bf16 images with ds_write_b128. The S
//     and PV phases keep their LDS reads, fragment layouts and mask arithmetic; the widening is
//     paid once per workgroup (16 codes per operand per thread per tile), not by each of the four
//     waves at read time.
//   * Widening is exact and carries no scale (e4m3x4_to_bf16): folding the scale in would round
//     code * scale to bf16. k_scale[key] multiplies the fp32 score before the masks and the
//     running max, v_scale[key] the fp32 probability before it is rounded to bf16 for the PV
//     operand; the row sum l takes the unscaled probability. The scales of a tile lie behind the
//     four images (per buffer KB k-scales, KB v-scales) and are read as broadcast ds_read_b128:
//     the four keys (e & 3) of a register group are consecutive positions.
//   * Redirected rows (past kend; a dead paged group) take their SCALE from the redirected
//     position too: a stale scale may be NaN, and 0 * NaN is NaN in the PV operand.
//   * Tile size: FwdGeo<D>::KB is kept (4 KiB of codes per operand per tile). The images in LDS
//     are bf16 either way, so doubling the keys per tile would double the LDS (66 KiB per
//     workgroup) and the score registers (the D = 128 forms already take 200 VGPRs, 2 waves per
//     SIMD) for global loads that are already a whole tile ahead of their use; keeping KB also
//     keeps the tile walk, the masks and the paged group bits those of the bf16 kernel.
#include "attn_tile.h"
#include "common.h"

namespace dlbb {

namespace {

constexpr float kPfNegBig = -1.0e30f;   // raw score of a masked key: finite

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct PrefillArgs {
  const uint16_t* qkv;      // [B, T, 3, H, D], token row stride ld
  const uint16_t* k_cache;  // [B, H, L_max, D]; Paged: the pool [n_pages, H, P, D]
  const uint16_t* v_cache;
  const int* length;
  uint16_t* out;            // [B, T, H, D], token row stride ldo
  int64_t ld, ldo;
  int B, T, H, L_max;
  float scale_log2;         // log2(e) * scale
  const int* table;         // Paged: [B, tstride]
  int64_t tstride;
  int n_pages, psh;         // P = 1 << psh
  const float* k_scale;     // Fp8: [B, H, L_max]; Paged: [n_pages, H, P]. The caches hold bytes
  const float* v_scale;
};

// 4 e4m3fn bytes (byte order) -> 4 bf16 (two words), exactly: v_cvt_pk_f32_fp8 is exact and an
// e4m3 value has 3 mantissa bits, so the low half of its fp32 form is zero and v_perm_b32 keeps
// the high halves. 4 VALU ops per 4 codes.
__device__ __forceinline__ u32x2 e4m3x4_to_bf16(uint32_t w) {
  const auto a = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(w), false);
  const auto b = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(w), true);
  return u32x2{__builtin_amdgcn_perm(__float_as_uint(a[1]), __float_as_uint(a[0]), 0x07060302u),
               __builtin_amdgcn_perm(__float_as_uint(b[1]), __float_as_uint(b[0]), 0x07060302u)};
}

// 16 codes -> the two 16-B chunks c0, c0 + 1 of image row `row_base` under swizzle `swz`
__device__ __forceinline__ void widen_store(const u32x4& codes, char* row_base, int c0, int swz) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const u32x2 lo = e4m3x4_to_bf16(codes[2 * i]), hi = e4m3x4_to_bf16(codes[2 * i + 1]);
    *reinterpret_cast<u32x4*>(row_base + (((c0 + i) ^ swz) << 4)) =
        u32x4{lo[0], lo[1], hi[0], hi[1]};
  }
}

template <int D, bool PerSeq, bool Paged, bool Fp8>
__global__ void __launch_bounds__(kAttnThreads, 2) attn_prefill_kernel(PrefillArgs a) {
  using G = FwdGeo<D>;
  constexpr int KB = G::KB, ROW = G::ROW, RPI = G::RPI, TILE = G::TILE;
  constexpr int WROWS = KB / 4;                   // image rows staged per wave
  constexpr int NG = KB / 16;                     // 16-key groups (paged: one page each) per tile
  constexpr unsigned kAllGroups = (1u << NG) - 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, hi = lane >> 5;
  int blk, h, b;
  head_block(1, blk, h, b);
  const int nqb = gridDim.x;
  const int q0 = (nqb - 1 - blk) * kQB;           // heaviest query block first
  const int qw = q0 + wave * 32;                  // this wave's first query
  const int qme = qw + r;                         // this lane's query
  const int hoff = h * D;
  int len;
  if constexpr (PerSeq) len = a.length[b];
  else len = *a.length;
  uint16_t* op = a.out + (static_cast<int64_t>(b) * a.T + qme) * a.ldo + hoff;
  if (len < 0) {                                  // empty slot: zero rows, nothing loaded
    if (qme < a.T) {
      const u16x4 z{0, 0, 0, 0};
#pragma unroll
      for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) *reinterpret_cast<u16x4*>(op + dt * 32 + 8 * gg + 4 * hi) = z;
    }
    return;
  }
  // cache positions that exist for this launch; the block's tiles cover its last query's keys
  const int kend = static_cast<int>(
      static_cast<int64_t>(len) + a.T < a.L_max ? static_cast<int64_t>(len) + a.T : a.L_max);
  const int qtop = q0 + kQB < a.T ? q0 + kQB : a.T;
  const int kmax = static_cast<int64_t>(len) + qtop < kend ? len + qtop : kend;
  const int nt = (kmax + KB - 1) / KB;
  const bool wave_live = qw < a.T;                // a wave past T only stages
  // last visible key of the lane's query / of the wave's first query (wave-uniform)
  const int64_t lq = static_cast<int64_t>(len) + qme;
  const int lim = lq < kend - 1 ? static_cast<int>(lq) : kend - 1;
  const int64_t lw = static_cast<int64_t>(len) + qw;
  const int wlim = lw < kend - 1 ? static_cast<int>(lw) : kend - 1;
  const int64_t wtop = lw + 31;                   // no key past it for any query of the wave

  // Q fragments (B operand of S^T = K Q^T): lane holds Q[qw + r][16 ks + 8 hi + j]
  bf16x8 qf[G::NKS];
  {
    const int q = qme < a.T ? qme : a.T - 1;
    const uint16_t* qp = a.qkv + (static_cast<int64_t>(b) * a.T + q) * a.ld + hoff + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < G::NKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + 16 * ks);
  }
  f32x16 o[G::NDT];
#pragma unroll
  for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = 0.5f * kPfNegBig * a.scale_log2, l = 0.f;

  auto tileK = [&](int c) { return smem + c * 2 * TILE; };
  auto tileV = [&](int c) { return smem + c * 2 * TILE + TILE; };

  // DMA: this lane stages image rows wave * WROWS + i * RPI + lane / (ROW / 16), i = 0, 1, chunk
  // slot ^ swz(row) of the cache row into slot `slot`. Contiguous: the sources of tile 0 kept,
  // tile kt adds k0 * D (uniform)
  const int r_in = lane / (ROW / 16), slot = lane % (ROW / 16);
  int kchunk[2], vchunk[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wave * WROWS + i * RPI + r_in;
    kchunk[i] = (slot ^ kswz_d<D>(row)) * 8;
    vchunk[i] = (slot ^ vswz_d<D>(row)) * 8;
  }
  [[maybe_unused]] const int64_t bh_row = (static_cast<int64_t>(b) * a.H + h) * a.L_max;
  [[maybe_unused]] const int* trow = Paged ? a.table + b * a.tstride : nullptr;
  // stages tile k0 into (tk, tv); returns the tile's group bits: low NG = mapped and live (a
  // group is live when its first position is below kend), next NG = live but NOT mapped
  auto stage = [&](int k0, char* tk, char* tv) -> unsigned {
    if constexpr (!Paged) {
      if (k0 + KB <= kend) {                       // wave-uniform: no row past kend
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int64_t e = (bh_row + k0 + wave * WROWS + i * RPI + r_in) * D;
          attn_glds16(a.k_cache + e + kchunk[i], tk + (wave * WROWS + i * RPI) * ROW);
          attn_glds16(a.v_cache + e + vchunk[i], tv + (wave * WROWS + i * RPI) * ROW);
        }
        return kAllGroups;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {                // rows past kend clamped (scores masked)
        int pos = k0 + wave * WROWS + i * RPI + r_in;
        pos = pos < kend ? pos : kend - 1;
        const int64_t e = (bh_row + pos) * D;
        attn_glds16(a.k_cache + e + kchunk[i], tk + (wave * WROWS + i * RPI) * ROW);
        attn_glds16(a.v_cache + e + vchunk[i], tv + (wave * WROWS + i * RPI) * ROW);
      }
      return kAllGroups;
    } else {
      int pg[NG];
      unsigned mp = 0, um = 0;
      int safe_pg = 0, safe_pos = 0;
#pragma unroll
      for (int g = NG - 1; g >= 0; --g) {          // descending: the FIRST mapped group is kept
        const int p0 = k0 + 16 * g;
        pg[g] = -1;
        if (p0 < kend) {                           // uniform: entries past the live range unread
          pg[g] = trow[p0 >> a.psh];
          if (pg[g] >= 0 && pg[g] < a.n_pages) {
            mp |= 1u << g;
            safe_pg = pg[g];
            safe_pos = p0;
          } else {
            um |= 1u << g;
          }
        }
      }
      if (mp == 0) return um << NG;                // nothing mapped: not loaded, not computed
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wave * WROWS + i * RPI + r_in;
        const int g = row >> 4;
        int pos = k0 + row;
        int page = pg[0];
#pragma unroll
        for (int j = 1; j < NG; ++j) page = g == j ? pg[j] : page;
        const bool ok = ((mp >> g) & 1u) && pos < kend;
        // a dead row re-reads the first position of the tile's first mapped live group
        page = ok ? page : safe_pg;
        pos = ok ? pos : safe_pos;
        const int64_t e = pool_row(page, a.H, h, a.psh, pos) * D;
        attn_glds16(a.k_cache + e + kchunk[i], tk + (wave * WROWS + i * RPI) * ROW);
        attn_glds16(a.v_cache + e + vchunk[i], tv + (wave * WROWS + i * RPI) * ROW);
      }
      return mp | (um << NG);
    }
  };

  // Fp8: a thread owns the 16-code run `frun` of tile row `frow` of K and of V (KB * D / 256 = 16
  // codes per operand), and the threads of runs 0 / 1 the row's k- / v-scale. fetch() issues the
  // global loads of tile k0 into registers (the row redirects and group bits are stage()'s) and
  // spill() widens them into the images of buffer c and puts the scales behind the four images:
  // per buffer KB k-scales, then KB v-scales. A redirected row takes its scales from the
  // redirected position too: a stale scale may be NaN and 0 * NaN is NaN in the PV operand.
  [[maybe_unused]] const int frow = threadIdx.x / (D / 16), frun = threadIdx.x % (D / 16);
  [[maybe_unused]] u32x4 kreg, vreg;
  [[maybe_unused]] float sreg = 0.f;
  auto tileS = [&](int c) { return reinterpret_cast<float*>(smem + 4 * TILE) + c * 2 * KB; };
  auto fetch = [&](int k0) -> unsigned {
    int64_t rowi;                                  // cache row: codes at rowi * D, scale at rowi
    unsigned bits = kAllGroups;
    if constexpr (!Paged) {
      const int pos = k0 + frow;
      rowi = bh_row + (pos < kend ? pos : kend - 1);
    } else {
      int pg[NG];
      unsigned mp = 0, um = 0;
      int safe_pg = 0, safe_pos = 0;
#pragma unroll
      for (int g = NG - 1; g >= 0; --g) {
        const int p0 = k0 + 16 * g;
        pg[g] = -1;
        if (p0 < kend) {
          pg[g] = trow[p0 >> a.psh];
          if (pg[g] >= 0 && pg[g] < a.n_pages) {
            mp |= 1u << g;
            safe_pg = pg[g];
            safe_pos = p0;
          } else {
            um |= 1u << g;
          }
        }
      }
      if (mp == 0) return um << NG;
      const int g = frow >> 4;
      int pos = k0 + frow;
      int page = pg[0];
#pragma unroll
      for (int j = 1; j < NG; ++j) page = g == j ? pg[j] : page;
      const bool ok = ((mp >> g) & 1u) && pos < kend;
      page = ok ? page : safe_pg;
      pos = ok ? pos : safe_pos;
      rowi = pool_row(page, a.H, h, a.psh, pos);
      bits = mp | (um << NG);
    }
    const int64_t e = rowi * D + 16 * frun;
    kreg = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint8_t*>(a.k_cache) + e);
    vreg = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint8_t*>(a.v_cache) + e);
    if (frun < 2) sreg = (frun ? a.v_scale : a.k_scale)[rowi];
    return bits;
  };
  auto spill = [&](int c) {
    widen_store(kreg, tileK(c) + frow * ROW, 2 * frun, kswz_d<D>(frow));
    widen_store(vreg, tileV(c) + frow * ROW, 2 * frun, vswz_d<D>(frow));
    if (frun < 2) tileS(c)[frun * KB + frow] = sreg;
  };

  unsigned gnext;
  if constexpr (Fp8) {
    gnext = fetch(0);
    if (gnext & kAllGroups) spill(0);
  } else {
    gnext = stage(0, tileK(0), tileV(0));
  }
  for (int kt = 0; kt < nt; ++kt) {
    const int cur = kt & 1;
    const unsigned gbits = gnext;
    // one barrier per tile: it both publishes tile kt (every wave's DMA retired; Fp8: every
    // wave's LDS writes) and frees buffer cur^1 (every wave finished tile kt-1), so the restage
    // goes right after it. Fp8: the loads of tile kt+1 are issued here and fly while tile kt is
    // computed; they are widened into buffer cur^1 after it
    if constexpr (Fp8) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 1 < nt) {
      if constexpr (Fp8) gnext = fetch((kt + 1) * KB);
      else gnext = stage((kt + 1) * KB, tileK(cur ^ 1), tileV(cur ^ 1));
    }
    const int k0 = kt * KB;
    // wave-uniform: the wave has queries, the tile a key one of them sees, and mapped rows
    if (wave_live && k0 <= wtop && (gbits & kAllGroups)) {
      const char* tk = tileK(cur);
      const char* tv = tileV(cur);
      // Fp8: the tile's scales, each batch read in one go ahead of its use (the k-scales under
      // the S MFMAs, the v-scales under the exponentials) so that no multiply waits on LDS alone.
      // The 4 keys (e & 3) of a register group are consecutive: one broadcast 16-B read
      [[maybe_unused]] f32x4 sc[G::NKK][4];
      [[maybe_unused]] auto read_scales = [&](const float* base) {
#pragma unroll
        for (int kk = 0; kk < G::NKK; ++kk)
#pragma unroll
          for (int q = 0; q < 4; ++q)
            sc[kk][q] = *reinterpret_cast<const f32x4*>(base + kk * 32 + 8 * q + 4 * hi);
      };
      if constexpr (Fp8) read_scales(tileS(cur));
      // ---- S^T for the 32-key halves
      f32x16 s[G::NKK];
#pragma unroll
      for (int kk = 0; kk < G::NKK; ++kk) {
#pragma unroll
        for (int e = 0; e < 16; ++e) s[kk][e] = 0.f;
        const int row = kk * 32 + r;
#pragma unroll
        for (int ks = 0; ks < G::NKS; ++ks) {
          const int c = 2 * ks + hi;
          const bf16x8 kf =
              *reinterpret_cast<const bf16x8*>(tk + row * ROW + ((c ^ kswz_d<D>(row)) << 4));
          s[kk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[kk], 0, 0, 0);
        }
      }
      // Fp8: the keys' scales on the fp32 scores, before the masks (a masked key's scale may be
      // stale); then the v-scales set off
      if constexpr (Fp8) {
#pragma unroll
        for (int kk = 0; kk < G::NKK; ++kk)
#pragma unroll
          for (int e = 0; e < 16; ++e) s[kk][e] *= sc[kk][e >> 2][e & 3];
        read_scales(tileS(cur) + KB);
      }
      // ---- masks (lane = one query; keys in registers), online softmax
      if (k0 + KB - 1 > wlim) {                     // some key of the tile beyond some query
        // key(kk, e) = k0 + 4 hi + kk*32 + (e & 3) + 8 (e >> 2): one per-lane threshold
        const int th = lim - k0 - 4 * hi;
#pragma unroll
        for (int kk = 0; kk < G::NKK; ++kk)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if (kk * 32 + (e & 3) + 8 * (e >> 2) > th) s[kk][e] = kPfNegBig;
      }
      if constexpr (Paged) {
        if (gbits >> NG) {                          // a live group on an unmapped page
          // key(kk, e) lies in group 2 kk + (e >> 3): a uniform test per 8 registers
#pragma unroll
          for (int kk = 0; kk < G::NKK; ++kk)
#pragma unroll
            for (int e = 0; e < 16; ++e)
              if ((gbits >> (NG + 2 * kk + (e >> 3))) & 1u) s[kk][e] = kPfNegBig;
        }
      }
      float mx = kPfNegBig;                          // max of the RAW scores (scale > 0)
#pragma unroll
      for (int kk = 0; kk < G::NKK; ++kk)
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[kk][e]);
      mx = xhalf_max(mx);
      // deferred max (as attn_fwd_kernel): the running max moves only when some lane's tile max
      // exceeds it by more than 2^8 in probability; a tile max of masked keys alone lies below
      // the starting max and never moves it
      const float mc = mx * a.scale_log2;
      const float mn = __any(mc > m + 8.f) ? fmaxf(m, mc) : m;
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      const bool rescale = m != mn;
      m = mn;
      float ls = 0.f;
#pragma unroll
      for (int kk = 0; kk < G::NKK; ++kk)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          s[kk][e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kk][e], a.scale_log2, -mn));
          ls += s[kk][e];
        }
      l = l * alpha + ls;
      if (__any(rescale)) {                          // wave-uniform skip when no max moved
#pragma unroll
        for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
          for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
      }
      // ---- O^T += V^T P^T: k-step = 16 keys;
      //      P^T element j <-> key 16 s + 8 (j>>2) + 4 hi + (j&3)
      const int g = lane >> 4, i16 = lane & 15;
      const int tq = i16 >> 2, tp = i16 & 3;        // tr-read lane role: block row / col group
#pragma unroll
      for (int kk = 0; kk < G::NKK; ++kk)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          bf16x8 pf;
          if constexpr (Fp8) {                       // v_scale[key] on the fp32 probability
#pragma unroll
            for (int j = 0; j < 8; ++j) s[kk][8 * st + j] *= sc[kk][2 * st + (j >> 2)][j & 3];
          }
#pragma unroll
          for (int j = 0; j < 8; ++j)
            pf[j] = __builtin_bit_cast(short, static_cast<__bf16>(s[kk][8 * st + j]));
#pragma unroll
          for (int dt = 0; dt < G::NDT; ++dt) {
            bf16x8 vf;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
              const int row = kk * 32 + 16 * st + 8 * half + 4 * (g >> 1) + tq;
              const int col = dt * 32 + 16 * (g & 1) + 4 * tp;
              const int off = row * ROW + (((col >> 3) ^ vswz_d<D>(row)) << 4) + (col & 7) * 2;
              // builtin read, as in attn_fwd_kernel (the asm form measured slower there)
              const i16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(tv + off));
#pragma unroll
              for (int u = 0; u < 4; ++u) vf[4 * half + u] = t[u];
            }
            o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
          }
        }
    }
    if constexpr (Fp8) {
      if (kt + 1 < nt && (gnext & kAllGroups)) spill(cur ^ 1);
    }
  }

  // ---- finalize: l over both lane halves, O / l, store O [B, T, H, D]
  const float lt = l + __shfl_xor(l, 32, 64);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  if (qme < a.T) {
#pragma unroll
    for (int dt = 0; dt < G::NDT; ++dt)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        u16x4 w;
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = f32_to_bf16(o[dt][4 * gg + u] * inv);
        *reinterpret_cast<u16x4*>(op + dt * 32 + 8 * gg + 4 * hi) = w;
      }
  }
}

bool mis(const void* p, uintptr_t n) { return reinterpret_cast<uintptr_t>(p) & (n - 1); }

// validation and the launch of the three entry points (table = null: a contiguous cache)
template <bool PerSeq, bool Paged, bool Fp8 = false>
int prefill_launch(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache,
                   const void* length, const void* table, int64_t tstride, int n_pages, int P,
                   void* out, int64_t ldo, int B, int T, int H, int D, int L_max, float scale,
                   hipStream_t stream, const void* k_scale = nullptr,
                   const void* v_scale = nullptr) {
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  if (B <= 0 || T <= 0 || H <= 0 || L_max <= 0 || !(scale > 0.f)) return hipErrorInvalidValue;
  if (!qkv || !k_cache || !v_cache || !out || !length) return hipErrorInvalidValue;
  if (Fp8 && (!k_scale || !v_scale || mis(k_scale, 4) || mis(v_scale, 4)))
    return hipErrorInvalidValue;
  if (ld % 8 || ld < 3 * H * D || ldo % 4 || ldo < H * D) return hipErrorInvalidValue;
  if (mis(qkv, 16) || mis(k_cache, 16) || mis(v_cache, 16) || mis(out, 8) || mis(length, 4))
    return hipErrorInvalidValue;
  if (H > 65535 || B > 65535) return hipErrorInvalidValue;
  int psh = 0;
  if (Paged) {
    if (!table || mis(table, 4) || n_pages <= 0) return hipErrorInvalidValue;
    if (P < 16 || P > 256 || (P & (P - 1))) return hipErrorInvalidValue;
    if (tstride < (static_cast<int64_t>(L_max) + P - 1) / P) return hipErrorInvalidValue;
    psh = __builtin_ctz(P);
  }
  PrefillArgs a{static_cast<const uint16_t*>(qkv), static_cast<const uint16_t*>(k_cache),
                static_cast<const uint16_t*>(v_cache), static_cast<const int*>(length),
                static_cast<uint16_t*>(out), ld, ldo, B, T, H, L_max,
                scale * 1.4426950408889634f, static_cast<const int*>(table), tstride, n_pages,
                psh, static_cast<const float*>(k_scale), static_cast<const float*>(v_scale)};
  const dim3 grid((T + kQB - 1) / kQB, H, B);
  // Fp8: 2 buffers x (KB k-scales + KB v-scales) behind the four images
  if (D == 64)
    hipLaunchKernelGGL((attn_prefill_kernel<64, PerSeq, Paged, Fp8>), grid, dim3(kAttnThreads),
                       4 * FwdGeo<64>::TILE + (Fp8 ? 16 * FwdGeo<64>::KB : 0), stream, a);
  else
    hipLaunchKernelGGL((attn_prefill_kernel<128, PerSeq, Paged, Fp8>), grid, dim3(kAttnThreads),
                       4 * FwdGeo<128>::TILE + (Fp8 ? 16 * FwdGeo<128>::KB : 0), stream, a);
  return hipGetLastError();
}

}  // namespace

}  // namespace dlbb

using namespace dlbb;

// qkv [B, T, 3, H, D] bf16 (token row stride ld), k_cache / v_cache [B, H, L_max, D] bf16
// contiguous, length: ONE device int32, out [B, T, H, D] bf16 (token row stride ldo). The T
// tokens' K / V are already in the cache at [*length, *length + T) (dlbb_kv_append) and *length
// is not advanced yet; query i attends positions 0 .. *length + i. Bad arguments (head dim,
// alignment, T < 1, L_max < 1, a null pointer) return hipErrorInvalidValue before any launch.
DLBB_API int dlbb_attn_prefill(const void* qkv, int64_t ld, const void* k_cache,
                               const void* v_cache, const void* length, void* out, int64_t ldo,
                               int B, int T, int H, int D, int L_max, float scale,
                               hipStream_t stream) {
  return prefill_launch<false, false>(qkv, ld, k_cache, v_cache, length, nullptr, 0, 0, 0, out,
                                      ldo, B, T, H, D, L_max, scale, stream);
}

// Per-sequence lengths: length is device int32[B], row b attends from length[b]; a row with
// length[b] < 0 is an empty slot: nothing loaded, zero rows out.
DLBB_API int dlbb_attn_prefill_seq(const void* qkv, int64_t ld, const void* k_cache,
                                   const void* v_cache, const void* length, void* out,
                                   int64_t ldo, int B, int T, int H, int D, int L_max,
                                   float scale, hipStream_t stream) {
  return prefill_launch<true, false>(qkv, ld, k_cache, v_cache, length, nullptr, 0, 0, 0, out,
                                     ldo, B, T, H, D, L_max, scale, stream);
}

// Paged pools k_pool / v_pool [n_pages, H, P, D], block_table device int32[B, table_stride] with
// table_stride >= ceil(L_max / P), P a power of two in [16, 256], length int32[B] under the _seq
// rules, L_max the logical cap. A key whose table entry lies outside [0, n_pages) is never
// addressed and never attended.
DLBB_API int dlbb_attn_prefill_paged(const void* qkv, int64_t ld, const void* k_pool,
                                     const void* v_pool, const void* length,
                                     const void* block_table, int64_t table_stride, int n_pages,
                                     int P, void* out, int64_t ldo, int B, int T, int H, int D,
                                     int L_max, float scale, hipStream_t stream) {
  return prefill_launch<true, true>(qkv, ld, k_pool, v_pool, length, block_table, table_stride,
                                    n_pages, P, out, ldo, B, T, H, D, L_max, scale, stream);
}

// The same over the FP8 cache (file header, "FP8 cache"): k_cache / v_cache [B, H, L_max, D]
// e4m3fn, k_scale / v_scale [B, H, L_max] fp32, as dlbb_kv_append_fp8 wrote them. The scales must
// be non-null and 4-byte aligned, the code pointers 16-byte aligned.
DLBB_API int dlbb_attn_prefill_fp8(const void* qkv, int64_t ld, const void* k_cache,
                                   const void* v_cache, const void* k_scale, const void* v_scale,
                                   const void* length, void* out, int64_t ldo, int B, int T,
                                   int H, int D, int L_max, float scale, hipStream_t stream) {
  return prefill_launch<false, false, true>(qkv, ld, k_cache, v_cache, length, nullptr, 0, 0, 0,
                                            out, ldo, B, T, H, D, L_max, scale, stream, k_scale,
                                            v_scale);
}

// The FP8 cache with per-sequence lengths (dlbb_attn_prefill_seq's rules).
DLBB_API int dlbb_attn_prefill_fp8_seq(const void* qkv, int64_t ld, const void* k_cache,
                                       const void* v_cache, const void* k_scale,
                                       const void* v_scale, const void* length, void* out,
                                       int64_t ldo, int B, int T, int H, int D, int L_max,
                                       float scale, hipStream_t stream) {
  return prefill_launch<true, false, true>(qkv, ld, k_cache, v_cache, length, nullptr, 0, 0, 0,
                                           out, ldo, B, T, H, D, L_max, scale, stream, k_scale,
                                           v_scale);
}

// The FP8 pools (dlbb_attn_prefill_paged's rules): k_pool / v_pool [n_pages, H, P, D] e4m3fn,
// k_scale / v_scale [n_pages, H, P] fp32. An entry outside [0, n_pages) becomes no address, for
// codes or for scales.
DLBB_API int dlbb_attn_prefill_fp8_paged(const void* qkv, int64_t ld, const void* k_pool,
                                         const void* v_pool, const void* k_scale,
                                         const void* v_scale, const void* length,
                                         const void* block_table, int64_t table_stride,
                                         int n_pages, int P, void* out, int64_t ldo, int B, int T,
                                         int H, int D, int L_max, float scale,
                                         hipStream_t stream) {
  return prefill_launch<true, true, true>(qkv, ld, k_pool, v_pool, length, block_table,
                                          table_stride, n_pages, P, out, ldo, B, T, H, D, L_max,
                                          scale, stream, k_scale, v_scale);
}
