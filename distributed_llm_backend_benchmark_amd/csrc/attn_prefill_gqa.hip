// Grouped-query chunked prefill: causal attention of a block of T new tokens over the grouped bf16
// KV cache, gfx950 (MI355X, CDNA4), head dim 64 / 128.
//
// Contract: attn_prefill.hip's on attn_decode_gqa.hip's layout. qkv is the block's fused
// activation [B, T, (H_q + 2 H_kv), D] bf16 (token row stride ld): the H_q query heads, then the
// H_kv key heads, then the H_kv value heads. Query head h uses KV head h / G, G = H_q / H_kv in
// {2, 4, 8, 16}. k_cache / v_cache are [B, H_kv, L_max, D] bf16 contiguous. The block's K / V rows
// were appended at [len_b, len_b + T) by dlbb_kv_append_gqa* BEFORE this launch and `length` has
// not been advanced: len_b is the word the append read (*length, or length[b] for the _seq form),
// read here from device memory too. Query i of row b attends cache positions 0 .. len_b + i (the
// causal mask is bottom-right aligned); EVERY key and value comes from the cache, only Q from
// qkv. Output [B, T, H_q * D] bf16 (row stride ldo), heads interleaved. No LSE, no workspace, no
// atomics: bit-identical from run to run. len_b < 0 is an empty slot: zero rows out, nothing
// loaded. Positions at or past kend = min(len_b + T, L_max) are never loaded (stale rows may hold
// NaN bit patterns, and 0 * NaN is NaN in the PV product): a tile row past kend is redirected to
// position kend - 1 and its score masked. A masked score is the finite -1e30 and the running max
// starts at half of it (scaled): no inf - inf, a lane without a visible key writes zeros.
//
// What is new is the ROW MAPPING; below it the kernel keeps attn_tile.h's geometry (4 waves, a
// lane owns one row of S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_32x32x16_bf16, 8-KiB K / V
// images staged by LDS-DMA and double buffered with one barrier per tile, ds_read_b128 /
// ds_read_b64_tr_b16 under kswz_d / vswz_d, the deferred running max).
//   * The 128 rows of a workgroup's query tile are (token, query head) pairs of ONE KV head. A
//     workgroup is (block, kvh, b) in a grid (ceil(T / TB), H_kv, B) with TB = 128 / G tokens per
//     block; row i = 32 wave + r is token t0 + (i >> log2 G) and query head kvh G + (i & (G - 1)).
//     A K / V tile staged once into LDS serves all G heads of the block's tokens, so the cache
//     is read once per KV head, not once per query head. A short block (the multi-token decode
//     step: T = 8 at G = 16) fills all 128 MFMA columns of one workgroup instead of leaving 8 live
//     rows in each of 16 workgroups that all stage the same prefix. At T G >= 128 the workgroups
//     and the MFMA work are the ungrouped kernel's at H = H_q over a cache G times smaller.
//   * Token-major rows: a wave spans NTW = 32 / G consecutive tokens, so its masked band is
//     KB + NTW keys, not KB + 32. Per wave: wlim, the limit of its first token (a tile is masked
//     only when it reaches past it), and wtop = len_b + first token + NTW - 1 (no key past it for
//     any row of the wave: later tiles are only staged). Per lane: the threshold
//     min(len_b + token(lane), kend - 1) - k0 - 4 hi.
//   * Q fragments are a per-lane gather: lane r loads qkv + (b T + token) ld + head D + 16 ks +
//     8 hi, 16 bytes each (the G heads of a token are G D contiguous elements, so 2 G lanes cover
//     a contiguous run per k-step). A token at or past T re-reads token T - 1 and is never stored.
//     The output is the matching scatter to out + (b T + token) ldo + head D.
//   * K / V sources: row * D of the [L_max, D] run of (b, kvh).
//   * Work order: token blocks run heaviest (last) first through head_block with H = H_kv, so the
//     blocks of a KV head sit behind one L2 and its prefix leaves HBM once.
//   * G is a launch argument (a shift), not a template parameter: the row mapping costs a few
//     integer ops per lane outside the key loop, and the file keeps four instantiations
//     (D x shared / per-sequence length).
// Sliding window (the Win instantiations, dlbb_attn_prefill_gqa_win*): token i of row b attends the
// last W keys, itself included: [max(0, len_b + i - W + 1), min(len_b + i, kend - 1)].
//   * The tile loop starts at the block's first useful tile, floor(max(0, len_b + t0 - W + 1) /
//     KB), from the block's FIRST token t0: workgroup-uniform, so every wave passes the same
//     barriers of the double-buffered staging. Tiles below it are neither staged nor computed, so
//     a short block over a long prefix walks the tiles of W + T keys and needs no key split.
//   * The low side mirrors the high side. Per wave: wbot, the lower bound of its first token (a
//     tile wholly below it is only staged), and wlow, that of its last token (a tile is masked on
//     the low side only when it reaches below it). Per lane: the threshold
//     max(0, len_b + token(lane) - W + 1) - k0 - 4 hi. Rows of a staged tile below a token's
//     bound are live cache rows, masked by the score.
//   * A row whose keys in a tile are all masked (its first visited tile can be, on the low side)
//     has a tile max of -1e30 below the half-start running max: the max does not move, alpha = 1,
//     p = 0. A token past the cache with no visible key ends with l = 0 and writes zeros.
//   * With W >= len_b + T every bound is 0 and the launch has the bits of the unwindowed kernel.
// Rotary position embedding (the Rope instantiations, dlbb_attn_prefill_gqa*_rope*; the table and
// the rotation are attn_tile.h's rope_rotate8): the lane that holds Q[tok][head][16 ks + 8 hi + j]
// holds the partner column 16 (ks + D / 32) + 8 hi + j too, so Q is rotated in registers right
// after the gather, at table row len_b + token(lane), the row at which dlbb_kv_append_gqa_rope*
// stored that token's K. A lane whose token is at or past T takes the row of token T - 1 with its
// values (inside the table, finite); a position at or past L_max takes row L_max - 1 (the table
// has L_max rows; such a token has no key of its own in the cache). Nothing in the tile loop
// differs.
// Not here: a split of the keys across workgroups (a short block over a long prefix runs
// H_kv B workgroups; under a window it visits the window's tiles only), paged and FP8 grouped
// caches.
#include "attn_tile.h"
#include "common.h"

namespace dlbb {

namespace {

constexpr float kPgNegBig = -1.0e30f;   // raw score of a masked key: finite

struct PrefillGqaArgs {
  const uint16_t* qkv;      // [B, T, H_q + 2 H_kv, D], token row stride ld
  const uint16_t* k_cache;  // [B, H_kv, L_max, D]
  const uint16_t* v_cache;
  const int* length;
  uint16_t* out;            // [B, T, H_q, D], token row stride ldo
  int64_t ld, ldo;
  int B, T, Hkv, L_max;
  int gsh;                  // log2 G
  float scale_log2;         // log2(e) * scale
  int window;               // Win kernels: keys a token attends, >= 1
  const float* rope;        // Rope kernels: cos | sin rows [>= L_max, D] fp32
};

template <int D, bool PerSeq, bool Win, bool Rope>
__global__ void __launch_bounds__(kAttnThreads, 2) attn_prefill_gqa_kernel(PrefillGqaArgs a) {
  using Geo = FwdGeo<D>;
  constexpr int KB = Geo::KB, ROW = Geo::ROW, RPI = Geo::RPI, TILE = Geo::TILE;
  constexpr int WROWS = KB / 4;                   // image rows staged per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, hi = lane >> 5;
  int blk, kvh, b;
  head_block(1, blk, kvh, b);
  const int gsh = a.gsh;
  const int TB = kQB >> gsh, NTW = 32 >> gsh;     // tokens per workgroup / per wave
  const int t0 = (gridDim.x - 1 - blk) * TB;      // heaviest token block first
  const int tw = t0 + wave * NTW;                 // this wave's first token
  const int tok = tw + (r >> gsh);                // this lane's token ...
  const int hoff = ((kvh << gsh) + (r & ((1 << gsh) - 1))) * D;   // ... and its query head
  int len;
  if constexpr (PerSeq) len = a.length[b];
  else len = *a.length;
  uint16_t* op = a.out + (static_cast<int64_t>(b) * a.T + tok) * a.ldo + hoff;
  if (len < 0) {                                  // empty slot: zero rows, nothing loaded
    if (tok < a.T) {
      const u16x4 z{0, 0, 0, 0};
#pragma unroll
      for (int dt = 0; dt < Geo::NDT; ++dt)
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) *reinterpret_cast<u16x4*>(op + dt * 32 + 8 * gg + 4 * hi) = z;
    }
    return;
  }
  // cache positions that exist for this launch; the block's tiles cover its last token's keys
  const int kend = static_cast<int>(
      static_cast<int64_t>(len) + a.T < a.L_max ? static_cast<int64_t>(len) + a.T : a.L_max);
  const int ttop = t0 + TB < a.T ? t0 + TB : a.T;
  const int kmax = static_cast<int64_t>(len) + ttop < kend ? len + ttop : kend;
  const int nt = (kmax + KB - 1) / KB;
  const bool wave_live = tw < a.T;                // a wave past T only stages
  // last visible key of the lane's token / of the wave's first token (wave-uniform)
  const int64_t lq = static_cast<int64_t>(len) + tok;
  const int lim = lq < kend - 1 ? static_cast<int>(lq) : kend - 1;
  const int64_t lw = static_cast<int64_t>(len) + tw;
  const int wlim = lw < kend - 1 ? static_cast<int>(lw) : kend - 1;
  const int64_t wtop = lw + NTW - 1;              // no key past it for any row of the wave
  // Win: the low side. llo: first key of the lane's token; wbot / wlow: of the wave's first / last
  // token (no row of the wave sees a key below wbot, none is masked at or above wlow); kt0: the
  // tile holding the first key of the block's first token. A token past T takes the bound of token
  // T - 1, so with a window over everything all four are 0 and no lane differs from the unwindowed
  // kernel. Without a window they are the constant 0
  int llo = 0, wbot = 0, wlow = 0, kt0 = 0;
  if constexpr (Win) {
    const int64_t last = static_cast<int64_t>(len) + a.T - 1;
    auto low = [&](int64_t p) {                   // first key of the token at cache position p
      const int64_t f = (p < last ? p : last) - a.window + 1;
      return static_cast<int>(f < 0 ? 0 : f < kend ? f : kend);
    };
    llo = low(lq);
    wbot = low(lw);
    wlow = low(wtop);
    kt0 = low(static_cast<int64_t>(len) + t0) / KB;
  }

  // Q fragments (B operand of S^T = K Q^T), gathered: lane holds Q[tok][head][16 ks + 8 hi + j]
  bf16x8 qf[Geo::NKS];
  {
    const int t = tok < a.T ? tok : a.T - 1;
    const uint16_t* qp = a.qkv + (static_cast<int64_t>(b) * a.T + t) * a.ld + hoff + 8 * hi;
#pragma unroll
    for (int ks = 0; ks < Geo::NKS; ++ks) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + 16 * ks);
    // Rope: k-step ks holds the low-half columns 16 ks + 8 hi + j, k-step ks + NKS / 2 their
    // partners; the table row is the cache position of the token that was loaded
    if constexpr (Rope) {
      const int64_t p = static_cast<int64_t>(len) + t;
      const float* cs = a.rope + (p < a.L_max ? p : a.L_max - 1) * D + 8 * hi;
#pragma unroll
      for (int ks = 0; ks < Geo::NKS / 2; ++ks)
        rope_rotate8(qf[ks], qf[ks + Geo::NKS / 2], cs + 16 * ks, D / 2);
    }
  }
  f32x16 o[Geo::NDT];
#pragma unroll
  for (int dt = 0; dt < Geo::NDT; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[dt][e] = 0.f;
  float m = 0.5f * kPgNegBig * a.scale_log2, l = 0.f;

  auto tileK = [&](int c) { return smem + c * 2 * TILE; };
  auto tileV = [&](int c) { return smem + c * 2 * TILE + TILE; };

  // DMA: this lane stages image rows wave * WROWS + i * RPI + lane / (ROW / 16), i = 0, 1, chunk
  // slot ^ swz(row) of the cache row into slot `slot`
  const int r_in = lane / (ROW / 16), slot = lane % (ROW / 16);
  int kchunk[2], vchunk[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = wave * WROWS + i * RPI + r_in;
    kchunk[i] = (slot ^ kswz_d<D>(row)) * 8;
    vchunk[i] = (slot ^ vswz_d<D>(row)) * 8;
  }
  const int64_t bh_row = (static_cast<int64_t>(b) * a.Hkv + kvh) * a.L_max;
  auto stage = [&](int k0, char* tk, char* tv) {
    const bool whole = k0 + KB <= kend;            // wave-uniform: no row past kend
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int pos = k0 + wave * WROWS + i * RPI + r_in;
      if (!whole) pos = pos < kend ? pos : kend - 1;   // rows past kend clamped (scores masked)
      const int64_t e = (bh_row + pos) * D;
      attn_glds16(a.k_cache + e + kchunk[i], tk + (wave * WROWS + i * RPI) * ROW);
      attn_glds16(a.v_cache + e + vchunk[i], tv + (wave * WROWS + i * RPI) * ROW);
    }
  };

  if (!Win || kt0 < nt) stage(kt0 * KB, tileK(kt0 & 1), tileV(kt0 & 1));
  for (int kt = kt0; kt < nt; ++kt) {
    const int cur = kt & 1;
    // one barrier per tile: it both publishes tile kt (every wave's DMA retired) and frees buffer
    // cur^1 (every wave finished tile kt-1), so the restage goes right after it
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 1 < nt) stage((kt + 1) * KB, tileK(cur ^ 1), tileV(cur ^ 1));
    const int k0 = kt * KB;
    // wave-uniform: the wave has tokens and the tile a key one of them sees
    if (wave_live && k0 <= wtop && k0 + KB > wbot) {
      const char* tk = tileK(cur);
      const char* tv = tileV(cur);
      // ---- S^T for the 32-key halves
      f32x16 s[Geo::NKK];
#pragma unroll
      for (int kk = 0; kk < Geo::NKK; ++kk) {
#pragma unroll
        for (int e = 0; e < 16; ++e) s[kk][e] = 0.f;
        const int row = kk * 32 + r;
#pragma unroll
        for (int ks = 0; ks < Geo::NKS; ++ks) {
          const int c = 2 * ks + hi;
          const bf16x8 kf =
              *reinterpret_cast<const bf16x8*>(tk + row * ROW + ((c ^ kswz_d<D>(row)) << 4));
          s[kk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[kk], 0, 0, 0);
        }
      }
      // ---- masks (lane = one (token, head) row; keys in registers), online softmax
      if (k0 + KB - 1 > wlim) {                     // some key of the tile beyond the first token
        // key(kk, e) = k0 + 4 hi + kk*32 + (e & 3) + 8 (e >> 2): one per-lane threshold
        const int th = lim - k0 - 4 * hi;
#pragma unroll
        for (int kk = 0; kk < Geo::NKK; ++kk)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if (kk * 32 + (e & 3) + 8 * (e >> 2) > th) s[kk][e] = kPgNegBig;
      }
      if constexpr (Win) {
        if (k0 < wlow) {                            // some key of the tile below the last token's
          const int tl = llo - k0 - 4 * hi;         // window: the same key index, from below
#pragma unroll
          for (int kk = 0; kk < Geo::NKK; ++kk)
#pragma unroll
            for (int e = 0; e < 16; ++e)
              if (kk * 32 + (e & 3) + 8 * (e >> 2) < tl) s[kk][e] = kPgNegBig;
        }
      }
      float mx = kPgNegBig;                          // max of the RAW scores (scale > 0)
#pragma unroll
      for (int kk = 0; kk < Geo::NKK; ++kk)
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[kk][e]);
      mx = xhalf_max(mx);
      // deferred max: the running max moves only when some lane's tile max exceeds it by more
      // than 2^8 in probability; a tile max of masked keys alone lies below the starting max
      const float mc = mx * a.scale_log2;
      const float mn = __any(mc > m + 8.f) ? fmaxf(m, mc) : m;
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      const bool rescale = m != mn;
      m = mn;
      float ls = 0.f;
#pragma unroll
      for (int kk = 0; kk < Geo::NKK; ++kk)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          s[kk][e] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kk][e], a.scale_log2, -mn));
          ls += s[kk][e];
        }
      l = l * alpha + ls;
      if (__any(rescale)) {                          // wave-uniform skip when no max moved
#pragma unroll
        for (int dt = 0; dt < Geo::NDT; ++dt)
#pragma unroll
          for (int e = 0; e < 16; ++e) o[dt][e] *= alpha;
      }
      // ---- O^T += V^T P^T: k-step = 16 keys;
      //      P^T element j <-> key 16 s + 8 (j>>2) + 4 hi + (j&3)
      const int g = lane >> 4, i16 = lane & 15;
      const int tq = i16 >> 2, tp = i16 & 3;        // tr-read lane role: block row / col group
#pragma unroll
      for (int kk = 0; kk < Geo::NKK; ++kk)
#pragma unroll
        for (int st = 0; st < 2; ++st) {
          bf16x8 pf;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            pf[j] = __builtin_bit_cast(short, static_cast<__bf16>(s[kk][8 * st + j]));
#pragma unroll
          for (int dt = 0; dt < Geo::NDT; ++dt) {
            bf16x8 vf;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
              const int row = kk * 32 + 16 * st + 8 * half + 4 * (g >> 1) + tq;
              const int col = dt * 32 + 16 * (g & 1) + 4 * tp;
              const int off = row * ROW + (((col >> 3) ^ vswz_d<D>(row)) << 4) + (col & 7) * 2;
              const i16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(tv + off));
#pragma unroll
              for (int u = 0; u < 4; ++u) vf[4 * half + u] = t[u];
            }
            o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, o[dt], 0, 0, 0);
          }
        }
    }
  }

  // ---- finalize: l over both lane halves, O / l, scatter O [B, T, H_q, D]
  const float lt = l + __shfl_xor(l, 32, 64);
  const float inv = lt > 0.f ? 1.f / lt : 0.f;
  if (tok < a.T) {
#pragma unroll
    for (int dt = 0; dt < Geo::NDT; ++dt)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        u16x4 w;
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = f32_to_bf16(o[dt][4 * gg + u] * inv);
        *reinterpret_cast<u16x4*>(op + dt * 32 + 8 * gg + 4 * hi) = w;
      }
  }
}

bool mis(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

// Win: `window` keys per token (>= 1; one that covers every token's prefix is no window). Rope:
// `rope` is the cos | sin table (fp32 [>= L_max, D], 16-byte aligned)
template <bool PerSeq, bool Win = false, bool Rope = false>
int prefill_gqa_launch(const void* qkv, int64_t ld, const void* k_cache, const void* v_cache,
                       const void* length, void* out, int64_t ldo, int B, int T, int Hq, int Hkv,
                       int D, int L_max, float scale, hipStream_t stream, int window = 0,
                       const void* rope = nullptr) {
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  if (Rope && (!rope || mis(rope, 16))) return hipErrorInvalidValue;
  if (Win && window < 1) return hipErrorInvalidValue;
  if (B <= 0 || T <= 0 || Hkv <= 0 || Hq <= 0 || L_max <= 0 || !(scale > 0.f))
    return hipErrorInvalidValue;
  if (Hq % Hkv) return hipErrorInvalidValue;
  const int G = Hq / Hkv;
  if (G != 2 && G != 4 && G != 8 && G != 16) return hipErrorInvalidValue;
  if (!qkv || !k_cache || !v_cache || !out || !length) return hipErrorInvalidValue;
  if (ld % 8 || ld < static_cast<int64_t>(Hq + 2 * Hkv) * D || ldo % 4 ||
      ldo < static_cast<int64_t>(Hq) * D)
    return hipErrorInvalidValue;
  if (mis(qkv, 16) || mis(k_cache, 16) || mis(v_cache, 16) || mis(out, 8) || mis(length, 4))
    return hipErrorInvalidValue;
  if (Hkv > 65535 || B > 65535) return hipErrorInvalidValue;
  const int gsh = __builtin_ctz(G);
  PrefillGqaArgs a{static_cast<const uint16_t*>(qkv), static_cast<const uint16_t*>(k_cache),
                   static_cast<const uint16_t*>(v_cache), static_cast<const int*>(length),
                   static_cast<uint16_t*>(out), ld, ldo, B, T, Hkv, L_max, gsh,
                   scale * 1.4426950408889634f, window, static_cast<const float*>(rope)};
  const int TB = kQB >> gsh;                       // tokens per workgroup
  const dim3 grid((T + TB - 1) / TB, Hkv, B);
  if (D == 64)
    hipLaunchKernelGGL((attn_prefill_gqa_kernel<64, PerSeq, Win, Rope>), grid, dim3(kAttnThreads),
                       4 * FwdGeo<64>::TILE, stream, a);
  else
    hipLaunchKernelGGL((attn_prefill_gqa_kernel<128, PerSeq, Win, Rope>), grid, dim3(kAttnThreads),
                       4 * FwdGeo<128>::TILE, stream, a);
  return hipGetLastError();
}

}  // namespace

}  // namespace dlbb

using namespace dlbb;

// qkv [B, T, H_q + 2 H_kv, D] bf16 (token row stride ld elements: H_q query heads, H_kv key heads,
// H_kv value heads), k_cache / v_cache [B, H_kv, L_max, D] bf16 contiguous, length: ONE device
// int32, out [B, T, H_q, D] bf16 (token row stride ldo). The T tokens' K / V are already in the
// cache at [*length, *length + T) (dlbb_kv_append_gqa) and *length is not advanced yet; query i of
// head h attends positions 0 .. *length + i of KV head h / (H_q / H_kv). Bad arguments (head dim
// outside {64, 128}, H_q / H_kv outside {2, 4, 8, 16} or not whole, B, T, H_kv or L_max < 1,
// scale <= 0, a null or misaligned pointer, ld or ldo too small or odd, H_kv or B above 65535)
// return hipErrorInvalidValue before any launch.
DLBB_API int dlbb_attn_prefill_gqa(const void* qkv, int64_t ld, const void* k_cache,
                                   const void* v_cache, const void* length, void* out,
                                   int64_t ldo, int B, int T, int Hq, int Hkv, int D, int L_max,
                                   float scale, hipStream_t stream) {
  return prefill_gqa_launch<false>(qkv, ld, k_cache, v_cache, length, out, ldo, B, T, Hq, Hkv, D,
                                   L_max, scale, stream);
}

// Per-sequence lengths: length is device int32[B], row b attends from length[b]; a row with
// length[b] < 0 is an empty slot: nothing loaded, zero rows out.
DLBB_API int dlbb_attn_prefill_gqa_seq(const void* qkv, int64_t ld, const void* k_cache,
                                       const void* v_cache, const void* length, void* out,
                                       int64_t ldo, int B, int T, int Hq, int Hkv, int D,
                                       int L_max, float scale, hipStream_t stream) {
  return prefill_gqa_launch<true>(qkv, ld, k_cache, v_cache, length, out, ldo, B, T, Hq, Hkv, D,
                                  L_max, scale, stream);
}

// Sliding window: dlbb_attn_prefill_gqa with `window` >= 1 keys per token. Query i of head h
// attends positions max(0, *length + i - window + 1) .. *length + i; the tiles below the first key
// of a workgroup's first token are neither staged nor computed. window < 1 returns
// hipErrorInvalidValue before any launch.
DLBB_API int dlbb_attn_prefill_gqa_win(const void* qkv, int64_t ld, const void* k_cache,
                                       const void* v_cache, const void* length, void* out,
                                       int64_t ldo, int B, int T, int Hq, int Hkv, int D,
                                       int L_max, int window, float scale, hipStream_t stream) {
  return prefill_gqa_launch<false, true>(qkv, ld, k_cache, v_cache, length, out, ldo, B, T, Hq,
                                         Hkv, D, L_max, scale, stream, window);
}

// The same with per-sequence lengths (dlbb_attn_prefill_gqa_seq's rules).
DLBB_API int dlbb_attn_prefill_gqa_win_seq(const void* qkv, int64_t ld, const void* k_cache,
                                           const void* v_cache, const void* length, void* out,
                                           int64_t ldo, int B, int T, int Hq, int Hkv, int D,
                                           int L_max, int window, float scale,
                                           hipStream_t stream) {
  return prefill_gqa_launch<true, true>(qkv, ld, k_cache, v_cache, length, out, ldo, B, T, Hq,
                                        Hkv, D, L_max, scale, stream, window);
}

// The rotary forms (the file header, "Rotary position embedding"): the entry points above with
// `rope`, the cos | sin table (fp32 [P >= L_max, D] contiguous, 16-byte aligned) after `length`.
// Query token t is rotated at table row *length + t (length[b] + t); the block's K must have been
// stored by dlbb_kv_append_gqa_rope* with the same table. A null or misaligned table returns
// hipErrorInvalidValue before any launch.
DLBB_API int dlbb_attn_prefill_gqa_rope(const void* qkv, int64_t ld, const void* k_cache,
                                        const void* v_cache, const void* length, const void* rope,
                                        void* out, int64_t ldo, int B, int T, int Hq, int Hkv,
                                        int D, int L_max, float scale, hipStream_t stream) {
  return prefill_gqa_launch<false, false, true>(qkv, ld, k_cache, v_cache, length, out, ldo, B, T,
                                                Hq, Hkv, D, L_max, scale, stream, 0, rope);
}

DLBB_API int dlbb_attn_prefill_gqa_rope_seq(const void* qkv, int64_t ld, const void* k_cache,
                                            const void* v_cache, const void* length,
                                            const void* rope, void* out, int64_t ldo, int B, int T,
                                            int Hq, int Hkv, int D, int L_max, float scale,
                                            hipStream_t stream) {
  return prefill_gqa_launch<true, false, true>(qkv, ld, k_cache, v_cache, length, out, ldo, B, T,
                                               Hq, Hkv, D, L_max, scale, stream, 0, rope);
}

DLBB_API int dlbb_attn_prefill_gqa_win_rope(const void* qkv, int64_t ld, const void* k_cache,
                                            const void* v_cache, const void* length,
                                            const void* rope, void* out, int64_t ldo, int B, int T,
                                            int Hq, int Hkv, int D, int L_max, int window,
                                            float scale, hipStream_t stream) {
  return prefill_gqa_launch<false, true, true>(qkv, ld, k_cache, v_cache, length, out, ldo, B, T,
                                               Hq, Hkv, D, L_max, scale, stream, window, rope);
}

DLBB_API int dlbb_attn_prefill_gqa_win_rope_seq(const void* qkv, int64_t ld, const void* k_cache,
                                                const void* v_cache, const void* length,
                                                const void* rope, void* out, int64_t ldo, int B,
                                                int T, int Hq, int Hkv, int D, int L_max,
                                                int window, float scale, hipStream_t stream) {
  return prefill_gqa_launch<true, true, true>(qkv, ld, k_cache, v_cache, length, out, ldo, B, T,
                                              Hq, Hkv, D, L_max, scale, stream, window, rope);
}
