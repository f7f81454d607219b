// Key-split grouped-query chunked prefill: attn_prefill_gqa.hip's attention of a block of T new
// tokens over the grouped bf16 KV cache, with the KEYS of a row cut into chunks of `chunk` keys
// that run in different workgroups (flash-decoding style), gfx950 (MI355X, CDNA4), head dim
// 64 / 128. For a short block over a long prefix (the verify step of speculative decoding, a
// second chat turn, the tail block of a chunked prompt) the unsplit kernel runs H_kv B workgroups
// that each walk the whole prefix serially; here the same prefix is n_chunks workgroups wide.
//
// Contract: attn_prefill_gqa.hip's, all of it (qkv [B, T, (H_q + 2 H_kv), D] bf16, caches
// [B, H_kv, L_max, D] bf16, the block appended at [len_b, len_b + T) before the launch and
// `length` not advanced, bottom-right causal mask read from the device length, len_b < 0 an empty
// slot (zero rows, nothing loaded), positions at or past kend = min(len_b + T, L_max) never loaded
// (redirected to kend - 1, score masked), a masked score the finite -1e30 and the starting max
// half of it, D in {64, 128}, G in {2, 4, 8, 16}). New:
//   * chunk: keys per workgroup, a positive multiple of 128 (a whole number of tiles at both tile
//     heights: KB = 64 at D 64, 32 at D 128).
//   * len_bound: the host's upper bound of max_b len_b + T, clamped to L_max here;
//     n_chunks = ceil(len_bound / chunk). The grids depend on shapes, len_bound and chunk only,
//     never on device data, so the launch pair can be captured.
//   * ws: fp32 [B, H_q, T, n_chunks, D + 2], per (row, chunk) the record m, l, o[D]; 64-bit
//     indexing. A record is written only by the workgroup that owns it and only when the row has a
//     visible key in the chunk; the combine reads exactly those records, so the workspace needs no
//     clearing and may hold anything (NaN included) elsewhere.
//
// Two kernels, no atomics, no counters, no "last workgroup combines":
//   attn_prefill_gqa_split_kernel    a workgroup is (chunk c, token block, kvh, b). It keeps the
//     unsplit kernel's row mapping and tile geometry (128 (token, query head) rows of one KV head,
//     4 waves, a lane owns one row of S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_32x32x16_bf16,
//     8-KiB K / V images by LDS-DMA, double buffered with one barrier per tile, the deferred
//     running max) and walks only the tiles of [c chunk, min((c + 1) chunk, kmax_block)). A
//     workgroup whose range is empty (a chunk past the block's last visible key, an empty slot)
//     exits at once and writes nothing. A tile is masked only when it reaches past the limit of
//     the wave's first token, so a chunk wholly inside the prefix runs the unmasked body. At the
//     end a lane adds its l over the two lane halves and stores m AS KEPT (the deferred running
//     max, scaled log2 domain), l and its fp32 o values UNNORMALISED: o and l are sums of
//     exp2(s - m) with that very m, so the merge by exp2(m_c - M) is exact whatever the deferred
//     update left. The o values go out as 16-byte vector stores (a record is 8-byte aligned: D + 2
//     is even, not a multiple of 4).
//   attn_prefill_gqa_combine_kernel  row (b, t, h), D / 4 lanes per row, 4 dims per lane. The live
//     chunks are 0 .. min(len_b + t, kend - 1) / chunk, capped at n_chunks; each holds a visible
//     key of the row (its first), so every l read is positive. Max of the m, then the merge in
//     chunk order in fp32, one division, bf16, out [B, T, H_q * D]. len_b < 0 writes zeros. The
//     order is fixed: bit-identical from run to run, and a row of a _seq launch has the bits of
//     its batch-1 shared-length launch at the same chunk and len_bound.
//
// Workgroup order and XCD placement. The split grid is (token blocks, n_chunks H_kv, B) run
// through attn_tile.h's head_block: every XCD takes a contiguous run of the order (b, kvh, chunk,
// token block) with the token block fastest. Token blocks of one chunk read the same tiles, sit
// next to each other in that order and so behind one L2: a chunk's K / V leave HBM once, not once
// per XCD. Different chunks share nothing and spread over the XCDs in runs. The blocks of a chunk
// therefore ask for the same tiles at nearly the same time, which docs/PERFORMANCE.md SUPPOSES is
// what costs the unsplit kernel 9 - 11 % at B 1; that supposition is neither confirmed nor tested
// here (no counter run, no placement A/B). The placement was chosen for the HBM volume at the
// shapes with several token blocks; at the shapes this kernel is for (T G <= 128) there is ONE
// token block per chunk and the question does not arise.
//
// Rotary position embedding (the Rope instantiations, dlbb_attn_prefill_gqa_split_rope*):
// attn_prefill_gqa.hip's rule. Every chunk's workgroup rotates its copy of Q in registers after the
// gather, at table row min(len_b + min(token(lane), T - 1), L_max - 1); the combine is unchanged.
//
// The tile body repeats attn_prefill_gqa.hip's.
#include "attn_tile.h"
#include "common.h"

namespace dlbb {

namespace {

constexpr float kPsNegBig = -1.0e30f;   // raw score of a masked key: finite
constexpr int kCombineThreads = 64;

// 16 bytes of fp32 at an 8-byte aligned address (a workspace record is D + 2 floats)
typedef float f32x4a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct PrefillGqaSplitArgs {
  const uint16_t* qkv;      // [B, T, H_q + 2 H_kv, D], token row stride ld
  const uint16_t* k_cache;  // [B, H_kv, L_max, D]
  const uint16_t* v_cache;
  const int* length;
  float* ws;                // [B, H_q, T, n_chunks, D + 2]: m, l, o[D]
  uint16_t* out;            // [B, T, H_q, D], token row stride ldo
  int64_t ld, ldo;
  int B, T, Hq, Hkv, L_max;
  int gsh;                  // log2 G
  int n_chunks, chunk;
  float scale_log2;         // log2(e) * scale
  const float* rope;        // Rope kernels: cos | sin rows [>= L_max, D] fp32
};

template <int D, bool PerSeq, bool Rope>
__global__ void __launch_bounds__(kAttnThreads, 2)
attn_prefill_gqa_split_kernel(PrefillGqaSplitArgs a) {
  using Geo = FwdGeo<D>;
  constexpr int KB = Geo::KB, ROW = Geo::ROW, RPI = Geo::RPI, TILE = Geo::TILE;
  constexpr int WROWS = KB / 4;                   // image rows staged per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, hi = lane >> 5;
  int blk, ch, b;
  head_block(1, blk, ch, b);                      // order (b, kvh, chunk, token block)
  const int c = ch % a.n_chunks, kvh = ch / a.n_chunks;
  int len;
  if constexpr (PerSeq) len = a.length[b];
  else len = *a.length;
  if (len < 0) return;                            // empty slot: the combine writes its zeros
  const int gsh = a.gsh;
  const int TB = kQB >> gsh, NTW = 32 >> gsh;     // tokens per workgroup / per wave
  const int t0 = (gridDim.x - 1 - blk) * TB;      // heaviest token block first
  // cache positions that exist for this launch; the block's keys end with its last token's
  const int kend = static_cast<int>(
      static_cast<int64_t>(len) + a.T < a.L_max ? static_cast<int64_t>(len) + a.T : a.L_max);
  const int ttop = t0 + TB < a.T ? t0 + TB : a.T;
  const int kmax = static_cast<int64_t>(len) + ttop < kend ? len + ttop : kend;
  const int klo = c * a.chunk;                    // < len_bound <= L_max
  if (klo >= kmax) return;                        // no key of this chunk is visible to the block
  const int khi = kmax - klo > a.chunk ? klo + a.chunk : kmax;
  const int kt0 = klo / KB, kt1 = (khi + KB - 1) / KB;   // klo is a multiple of 128

  const int tw = t0 + wave * NTW;                 // this wave's first token
  const int tok = tw + (r >> gsh);                // this lane's token ...
  const int head = (kvh << gsh) + (r & ((1 << gsh) - 1));   // ... and its query head
  const bool wave_live = tw < a.T;                // a wave past T only stages
  // last visible key of the lane's token / of the wave's first token (wave-uniform)
  const int64_t lq = static_cast<int64_t>(len) + tok;
  const int lim = lq < kend - 1 ? static_cast<int>(lq) : kend - 1;
  const int64_t lw = static_cast<int64_t>(len) + tw;
  const int wlim = lw < kend - 1 ? static_cast<int>(lw) : kend - 1;
  const int64_t wtop = lw + NTW - 1;              // no key past it for any row of the wave

  // Q fragments (B operand of S^T = K Q^T), gathered: lane holds Q[tok][head][16 ks + 8 hi + j]
  bf16x8 qf[Geo::NKS];
  {
    const int t = tok < a.T ? tok : a.T - 1;
    const uint16_t* qp = a.qkv + (static_cast<int64_t>(b) * a.T + t) * a.ld + head * D + 8 * hi;
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
  float m = 0.5f * kPsNegBig * a.scale_log2, l = 0.f;

  auto tileK = [&](int i) { return smem + i * 2 * TILE; };
  auto tileV = [&](int i) { return smem + i * 2 * TILE + TILE; };

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

  stage(kt0 * KB, tileK(0), tileV(0));
  for (int kt = kt0; kt < kt1; ++kt) {
    const int cur = (kt - kt0) & 1;
    // one barrier per tile: it both publishes tile kt (every wave's DMA retired) and frees buffer
    // cur^1 (every wave finished tile kt-1), so the restage goes right after it
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + 1 < kt1) stage((kt + 1) * KB, tileK(cur ^ 1), tileV(cur ^ 1));
    const int k0 = kt * KB;
    // wave-uniform: the wave has tokens and the tile a key one of them sees
    if (wave_live && k0 <= wtop) {
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
          const int cc = 2 * ks + hi;
          const bf16x8 kf =
              *reinterpret_cast<const bf16x8*>(tk + row * ROW + ((cc ^ kswz_d<D>(row)) << 4));
          s[kk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s[kk], 0, 0, 0);
        }
      }
      // ---- masks (lane = one (token, head) row; keys in registers), online softmax. Keys at or
      // past khi = kmax in the block's last tile lie past every row's limit, so this covers them
      if (k0 + KB - 1 > wlim) {                     // some key of the tile beyond the first token
        // key(kk, e) = k0 + 4 hi + kk*32 + (e & 3) + 8 (e >> 2): one per-lane threshold
        const int th = lim - k0 - 4 * hi;
#pragma unroll
        for (int kk = 0; kk < Geo::NKK; ++kk)
#pragma unroll
          for (int e = 0; e < 16; ++e)
            if (kk * 32 + (e & 3) + 8 * (e >> 2) > th) s[kk][e] = kPsNegBig;
      }
      float mx = kPsNegBig;                          // max of the RAW scores (scale > 0)
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

  // ---- the partial of (row, chunk): m as kept, l over both lane halves, o unnormalised. Only a
  // row with a visible key in the chunk (its first: klo <= lim) has a record; its wave ran the
  // tile of klo, so l > 0 and m is a real score's
  const float lt = l + __shfl_xor(l, 32, 64);
  if (tok < a.T && lim >= klo) {
    float* wp = a.ws + (((static_cast<int64_t>(b) * a.Hq + head) * a.T + tok) * a.n_chunks + c) *
                           (D + 2);
    if (hi == 0) *reinterpret_cast<f32x2*>(wp) = f32x2{m, lt};
#pragma unroll
    for (int dt = 0; dt < Geo::NDT; ++dt)
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        const f32x4a8 w{o[dt][4 * gg], o[dt][4 * gg + 1], o[dt][4 * gg + 2], o[dt][4 * gg + 3]};
        *reinterpret_cast<f32x4a8*>(wp + 2 + dt * 32 + 8 * gg + 4 * hi) = w;
      }
  }
}

// One row (b, t, h) per D / 4 lanes, 4 output dims per lane.
template <int D, bool PerSeq>
__global__ void __launch_bounds__(kCombineThreads)
attn_prefill_gqa_combine_kernel(PrefillGqaSplitArgs a) {
  constexpr int TPR = D / 4, RPB = kCombineThreads / TPR;   // lanes per row, rows per workgroup
  const int64_t row = static_cast<int64_t>(blockIdx.x) * RPB + threadIdx.x / TPR;
  if (row >= static_cast<int64_t>(a.B) * a.T * a.Hq) return;
  const int q = threadIdx.x % TPR;
  const int h = static_cast<int>(row % a.Hq);
  const int64_t bt = row / a.Hq;
  const int t = static_cast<int>(bt % a.T), b = static_cast<int>(bt / a.T);
  int len;
  if constexpr (PerSeq) len = a.length[b];
  else len = *a.length;
  uint16_t* op = a.out + bt * a.ldo + h * D + 4 * q;
  if (len < 0) {                                  // empty slot: zero rows
    *reinterpret_cast<u16x4*>(op) = u16x4{0, 0, 0, 0};
    return;
  }
  const int kend = static_cast<int>(
      static_cast<int64_t>(len) + a.T < a.L_max ? static_cast<int64_t>(len) + a.T : a.L_max);
  const int64_t lq = static_cast<int64_t>(len) + t;
  const int lim = lq < kend - 1 ? static_cast<int>(lq) : kend - 1;
  int live = lim / a.chunk + 1;                   // chunks holding a visible key of the row
  live = live < a.n_chunks ? live : a.n_chunks;
  const float* p = a.ws + ((static_cast<int64_t>(b) * a.Hq + h) * a.T + t) * a.n_chunks * (D + 2);
  float mx = p[0];
  for (int c = 1; c < live; ++c) mx = fmaxf(mx, p[static_cast<int64_t>(c) * (D + 2)]);
  float lsum = 0.f;
  f32x4 acc{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < live; ++c) {                // fixed order: bit-identical from run to run
    const float* pc = p + static_cast<int64_t>(c) * (D + 2);
    const f32x2 ml = *reinterpret_cast<const f32x2*>(pc);
    const f32x4a8 oc = *reinterpret_cast<const f32x4a8*>(pc + 2 + 4 * q);
    const float f = __builtin_amdgcn_exp2f(ml[0] - mx);
    lsum = __builtin_fmaf(ml[1], f, lsum);
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(oc[u], f, acc[u]);
  }
  const float inv = 1.f / lsum;
  u16x4 w;
#pragma unroll
  for (int u = 0; u < 4; ++u) w[u] = f32_to_bf16(acc[u] * inv);
  *reinterpret_cast<u16x4*>(op) = w;
}

bool mis(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

// Rope: `rope` is the cos | sin table (fp32 [>= L_max, D], 16-byte aligned)
template <bool PerSeq, bool Rope = false>
int prefill_gqa_split_launch(const void* qkv, int64_t ld, const void* k_cache,
                             const void* v_cache, const void* length, void* ws, void* out,
                             int64_t ldo, int B, int T, int Hq, int Hkv, int D, int L_max,
                             int len_bound, int chunk, float scale, hipStream_t stream,
                             const void* rope = nullptr) {
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  if (Rope && (!rope || mis(rope, 16))) return hipErrorInvalidValue;
  if (B <= 0 || T <= 0 || Hkv <= 0 || Hq <= 0 || L_max <= 0 || !(scale > 0.f))
    return hipErrorInvalidValue;
  if (Hq % Hkv) return hipErrorInvalidValue;
  const int G = Hq / Hkv;
  if (G != 2 && G != 4 && G != 8 && G != 16) return hipErrorInvalidValue;
  if (chunk <= 0 || chunk % 128 || len_bound <= 0) return hipErrorInvalidValue;
  if (!qkv || !k_cache || !v_cache || !out || !length || !ws) return hipErrorInvalidValue;
  if (ld % 8 || ld < static_cast<int64_t>(Hq + 2 * Hkv) * D || ldo % 4 ||
      ldo < static_cast<int64_t>(Hq) * D)
    return hipErrorInvalidValue;
  if (mis(qkv, 16) || mis(k_cache, 16) || mis(v_cache, 16) || mis(out, 8) || mis(length, 4) ||
      mis(ws, 16))
    return hipErrorInvalidValue;
  const int bound = len_bound < L_max ? len_bound : L_max;
  const int n_chunks = (bound - 1) / chunk + 1;
  const int gsh = __builtin_ctz(G);
  const int TB = kQB >> gsh;                       // tokens per workgroup
  const int nblk = (T + TB - 1) / TB;
  const int64_t rows = static_cast<int64_t>(B) * T * Hq;
  constexpr int64_t kMaxGrid = 0x7fffffff;
  // grid limits: y and z of the split grid, head_block's 32-bit linear id, x of the combine grid
  if (static_cast<int64_t>(n_chunks) * Hkv > 65535 || B > 65535 ||
      static_cast<int64_t>(nblk) * n_chunks * Hkv * B > kMaxGrid || rows > kMaxGrid)
    return hipErrorInvalidValue;
  PrefillGqaSplitArgs a{static_cast<const uint16_t*>(qkv), static_cast<const uint16_t*>(k_cache),
                        static_cast<const uint16_t*>(v_cache), static_cast<const int*>(length),
                        static_cast<float*>(ws), static_cast<uint16_t*>(out), ld, ldo, B, T, Hq,
                        Hkv, L_max, gsh, n_chunks, chunk, scale * 1.4426950408889634f,
                        static_cast<const float*>(rope)};
  const dim3 grid(nblk, n_chunks * Hkv, B);
  const int rpb = kCombineThreads / (D / 4);
  const dim3 cgrid(static_cast<unsigned>((rows + rpb - 1) / rpb));
  if (D == 64) {
    hipLaunchKernelGGL((attn_prefill_gqa_split_kernel<64, PerSeq, Rope>), grid, dim3(kAttnThreads),
                       4 * FwdGeo<64>::TILE, stream, a);
    hipLaunchKernelGGL((attn_prefill_gqa_combine_kernel<64, PerSeq>), cgrid,
                       dim3(kCombineThreads), 0, stream, a);
  } else {
    hipLaunchKernelGGL((attn_prefill_gqa_split_kernel<128, PerSeq, Rope>), grid, dim3(kAttnThreads),
                       4 * FwdGeo<128>::TILE, stream, a);
    hipLaunchKernelGGL((attn_prefill_gqa_combine_kernel<128, PerSeq>), cgrid,
                       dim3(kCombineThreads), 0, stream, a);
  }
  return hipGetLastError();
}

}  // namespace

}  // namespace dlbb

using namespace dlbb;

// dlbb_attn_prefill_gqa's arguments and contract (attn_prefill_gqa.hip) with the keys split over
// workgroups. ws: fp32 [B, H_q, T, n_chunks, D + 2], 16-byte aligned, n_chunks =
// ceil(min(len_bound, L_max) / chunk); it needs no clearing. len_bound: the host's upper bound of
// *length + T (keys past it are not attended). chunk: keys per workgroup, a positive multiple of
// 128. Bad arguments (those of dlbb_attn_prefill_gqa, a chunk that is no positive multiple of 128,
// len_bound < 1, a null or misaligned ws, n_chunks H_kv above 65535, 2^31 or more split
// workgroups or output rows) return hipErrorInvalidValue before any launch.
DLBB_API int dlbb_attn_prefill_gqa_split(const void* qkv, int64_t ld, const void* k_cache,
                                         const void* v_cache, const void* length, void* ws,
                                         void* out, int64_t ldo, int B, int T, int Hq, int Hkv,
                                         int D, int L_max, int len_bound, int chunk, float scale,
                                         hipStream_t stream) {
  return prefill_gqa_split_launch<false>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B, T, Hq,
                                         Hkv, D, L_max, len_bound, chunk, scale, stream);
}

// Per-sequence lengths: length is device int32[B], row b attends from length[b] and len_bound
// bounds max_b length[b] + T; a row with length[b] < 0 is an empty slot: nothing loaded, zero
// rows out.
DLBB_API int dlbb_attn_prefill_gqa_split_seq(const void* qkv, int64_t ld, const void* k_cache,
                                             const void* v_cache, const void* length, void* ws,
                                             void* out, int64_t ldo, int B, int T, int Hq,
                                             int Hkv, int D, int L_max, int len_bound, int chunk,
                                             float scale, hipStream_t stream) {
  return prefill_gqa_split_launch<true>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B, T, Hq,
                                        Hkv, D, L_max, len_bound, chunk, scale, stream);
}

// The rotary forms (the file header, "Rotary position embedding"): the entry points above with
// `rope`, the cos | sin table (fp32 [P >= L_max, D] contiguous, 16-byte aligned) after `length`.
// Query token t is rotated at table row *length + t (length[b] + t); the block's K must have been
// stored by dlbb_kv_append_gqa_rope* with the same table. A null or misaligned table returns
// hipErrorInvalidValue before any launch.
DLBB_API int dlbb_attn_prefill_gqa_split_rope(const void* qkv, int64_t ld, const void* k_cache,
                                              const void* v_cache, const void* length,
                                              const void* rope, void* ws, void* out, int64_t ldo,
                                              int B, int T, int Hq, int Hkv, int D, int L_max,
                                              int len_bound, int chunk, float scale,
                                              hipStream_t stream) {
  return prefill_gqa_split_launch<false, true>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B,
                                               T, Hq, Hkv, D, L_max, len_bound, chunk, scale,
                                               stream, rope);
}

DLBB_API int dlbb_attn_prefill_gqa_split_rope_seq(const void* qkv, int64_t ld,
                                                  const void* k_cache, const void* v_cache,
                                                  const void* length, const void* rope, void* ws,
                                                  void* out, int64_t ldo, int B, int T, int Hq,
                                                  int Hkv, int D, int L_max, int len_bound,
                                                  int chunk, float scale, hipStream_t stream) {
  return prefill_gqa_split_launch<true, true>(qkv, ld, k_cache, v_cache, length, ws, out, ldo, B,
                                              T, Hq, Hkv, D, L_max, len_bound, chunk, scale,
                                              stream, rope);
}
