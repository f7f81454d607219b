// Single-query (decode) attention over a KV cache, gfx950 (MI355X, CDNA4).
//
// Cache layout, per layer and rank: k_cache / v_cache [B, H, L_max, D] bf16, contiguous, so the
// key stream of one (b, h) is one contiguous run; `length` is ONE device int32 = tokens already
// cached, shared by the batch (and by every layer). Every kernel here reads it from device
// memory, so a step captured in a HIP graph replays for successive positions.
//
//   kv_append_kernel           K / V rows of a fused qkv [B, T, 3, H, D] -> cache positions
//                              [length, length + T), 16-byte loads and stores.
//   attn_decode_split_kernel   grid (n_chunks, H, B): workgroup (c, h, b) attends the one query
//                              of (b, h) over keys [c * chunk, min((c + 1) * chunk, L)),
//                              L = length + 1 (the cached tokens and the token being decoded),
//                              and writes the partial (m, l, o[D]) in fp32 to the workspace.
//   attn_decode_combine_kernel one workgroup per (b, h): merges the live chunks' partials in
//                              chunk order and writes bf16 [B, 1, H * D] (heads interleaved).
//
// The split kernel is a bandwidth-bound read: K and V go from global memory straight into
// VGPRs, 16 bytes per lane, D / 8 lanes per key (a wave reads 1 KiB of consecutive key rows per
// load instruction); the dot product is reduced over those D / 8 lanes with shuffles. Each
// group of D / 8 lanes (a "slot") keeps an online softmax of its own over the keys it walks
// (fp32 running max m, sum l, and its 8 columns of o); slots are merged once at the end, inside
// the wave by shuffles and across the 4 waves through LDS, in a fixed order. No MFMA, no LDS
// staging of K / V, no atomics, no tickets: results are bit-identical from run to run.
//
// `fused` = 1: the chunk that owns position `length` takes the new token's K / V from `qkv` and
// also writes them to the cache, so append + attend is one launch; 0: the caller appended first
// (dlbb_kv_append) and every key is read from the cache.
#include "common.h"

namespace dlbb {

constexpr int kDecThreads = 256;
constexpr int kDecUnroll = 4;          // keys in flight per slot (8 x 16 B loads per lane)
constexpr float kDecNegBig = -1.0e30f; // "no key yet": finite, so no inf - inf in the merges

struct KvAppendArgs {
  const uint16_t* qkv;   // [B, T, 3, H, D], token row stride ld
  uint16_t* k_cache;     // [B, H, L_max, D]
  uint16_t* v_cache;
  const int* length;
  int64_t ld;
  int B, T, H, D, L_max;
};

// one 16-byte vector per thread step: (b, t, k|v, h, piece)
__global__ __launch_bounds__(256) void kv_append_kernel(KvAppendArgs a) {
  const int len = *a.length;
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
    const int64_t pos = static_cast<int64_t>(len) + t;
    if (len < 0 || pos >= a.L_max) continue;                // device-side guard: never past the cache
    const u16x8 val = *reinterpret_cast<const u16x8*>(
        a.qkv + (static_cast<int64_t>(b) * a.T + t) * a.ld + static_cast<int64_t>(1 + kv) * a.H * a.D +
        hp * 8);
    uint16_t* dst = (kv ? a.v_cache : a.k_cache) +
                    ((static_cast<int64_t>(b) * a.H + h) * a.L_max + pos) * a.D + piece * 8;
    *reinterpret_cast<u16x8*>(dst) = val;
  }
}

struct DecodeArgs {
  const uint16_t* qkv;   // [B, 1, 3, H, D], batch row stride ld
  uint16_t* k_cache;     // [B, H, L_max, D]
  uint16_t* v_cache;
  const int* length;
  float* ws;             // [B, H, n_chunks, D + 2]: m, l, o[D]
  uint16_t* out;         // [B, 1, H, D], batch row stride ldo
  int64_t ld, ldo;
  int B, H, L_max, chunk, n_chunks, fused;
  float scale_log2;
};

// keys the step attends (and whether the new token has a cache slot): uniform, from device memory
__device__ __forceinline__ int decode_keys(const DecodeArgs& a, int& len, bool& room) {
  len = *a.length;
  if (len < 0) len = 0;
  room = len < a.L_max;
  return room ? len + 1 : a.L_max;
}

__device__ __forceinline__ void bf16x8_to_f32(const u16x8& r, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = bf16_to_f32(r[j]);
}

template <int D>
__global__ __launch_bounds__(kDecThreads) void attn_decode_split_kernel(DecodeArgs a) {
  constexpr int LPK = D / 8;                 // lanes per key (16 B each)
  constexpr int NS = kDecThreads / LPK;      // key slots per workgroup
  constexpr int U = kDecUnroll;
  __shared__ float red[kDecThreads / kWave][D + 2];

  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  int len;
  bool room;
  const int L = decode_keys(a, len, room);
  const int k0 = c * a.chunk;
  if (k0 >= L) return;                       // dead chunk: no K / V read, no partial written
  const int k1 = min(k0 + a.chunk, L);
  const int tid = threadIdx.x, sub = tid % LPK, slot = tid / LPK;
  // position whose K / V come from qkv (and are stored to the cache here); -1: none
  const int newpos = (a.fused && room) ? len : -1;

  const uint16_t* row = a.qkv + static_cast<int64_t>(b) * a.ld + h * D + sub * 8;
  const uint16_t* nk = row + a.H * D;
  const uint16_t* nv = row + 2 * a.H * D;
  float q[8];
  bf16x8_to_f32(*reinterpret_cast<const u16x8*>(row), q);
  const int64_t base = (static_cast<int64_t>(b) * a.H + h) * a.L_max * D + sub * 8;
  uint16_t* kc = a.k_cache + base;
  uint16_t* vc = a.v_cache + base;

  float m = kDecNegBig, l = 0.f, o[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.f;

  for (int it = k0; it < k1; it += NS * U) {       // uniform trip count over the workgroup
    u16x8 kr[U], vr[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = it + u * NS + slot;
      ok[u] = key < k1;
      const int kk = ok[u] ? key : k1 - 1;         // masked slots re-read a live row
      const bool fresh = kk == newpos;
      kr[u] = *reinterpret_cast<const u16x8*>(fresh ? nk : kc + static_cast<int64_t>(kk) * D);
      vr[u] = *reinterpret_cast<const u16x8*>(fresh ? nv : vc + static_cast<int64_t>(kk) * D);
      if (fresh && ok[u]) {                        // the append, by the chunk owning `length`
        *reinterpret_cast<u16x8*>(kc + static_cast<int64_t>(kk) * D) = kr[u];
        *reinterpret_cast<u16x8*>(vc + static_cast<int64_t>(kk) * D) = vr[u];
      }
    }
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      bf16x8_to_f32(kr[u], kf);
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) d = __builtin_fmaf(q[j], kf[j], d);
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) d += __shfl_xor(d, off, 64);
      s[u] = ok[u] ? d * a.scale_log2 : kDecNegBig;
    }
    float mn = m;
#pragma unroll
    for (int u = 0; u < U; ++u) mn = fmaxf(mn, s[u]);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    l *= alpha;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= alpha;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = ok[u] ? __builtin_amdgcn_exp2f(s[u] - mn) : 0.f;
      float vf[8];
      bf16x8_to_f32(vr[u], vf);
      l += p;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = __builtin_fmaf(p, vf[j], o[j]);
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
    for (int j = 0; j < 8; ++j) {
      const float o2 = __shfl_xor(o[j], off, 64);
      const float oa = lo ? o[j] * f1 : o2 * f2, ob = lo ? o2 * f2 : o[j] * f1;
      o[j] = oa + ob;
    }
    m = mn;
  }
  const int lane = tid & (kWave - 1), w = tid / kWave;
  if (lane < LPK) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[w][sub * 8 + j] = o[j];
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
template <int D>
__global__ __launch_bounds__(D) void attn_decode_combine_kernel(DecodeArgs a) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  int len;
  bool room;
  const int L = decode_keys(a, len, room);
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

static bool mis16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace dlbb

using namespace dlbb;

// qkv: [B, T, 3, H, D] bf16 (token row stride ld elements); k_cache / v_cache: [B, H, L_max, D]
// bf16 contiguous; length: device int32. Rows K / V of every token go to cache positions
// [*length, *length + T); positions >= L_max are dropped on the device.
DLBB_API int dlbb_kv_append(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                            const void* length, int B, int T, int H, int D, int L_max,
                            hipStream_t stream) {
  if (B <= 0 || T <= 0 || H <= 0) return hipSuccess;
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  if (L_max <= 0 || ld % 8 || ld < 3 * H * D || !length) return hipErrorInvalidValue;
  if (mis16(qkv) || mis16(k_cache) || mis16(v_cache)) return hipErrorInvalidValue;
  KvAppendArgs a{static_cast<const uint16_t*>(qkv), static_cast<uint16_t*>(k_cache),
                 static_cast<uint16_t*>(v_cache), static_cast<const int*>(length), ld, B, T, H, D,
                 L_max};
  const int64_t vecs = static_cast<int64_t>(B) * T * 2 * H * (D / 8);
  hipLaunchKernelGGL(kv_append_kernel, dim3(stream_grid(vecs, 256)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// One decode step of attention: qkv [B, 1, 3, H, D] (batch row stride ld), the cache as above,
// out [B, 1, H, D] bf16 (batch row stride ldo). Attends over *length + 1 keys; with fused != 0
// the new token's K / V are taken from qkv and stored at position *length by the same launch,
// else the caller has appended them already. ws: fp32 [B, H, n_chunks, D + 2], n_chunks =
// ceil(min(len_bound, L_max) / chunk); len_bound is the host's upper bound of *length + 1.
DLBB_API int dlbb_attn_decode(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                              const void* length, void* ws, void* out, int64_t ldo, int B, int H,
                              int D, int L_max, int len_bound, int chunk, int fused, float scale,
                              hipStream_t stream) {
  if (B <= 0 || H <= 0) return hipSuccess;
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  if (L_max <= 0 || chunk <= 0 || len_bound <= 0 || !length || !ws) return hipErrorInvalidValue;
  if (ld % 8 || ld < 3 * H * D || ldo < H * D) return hipErrorInvalidValue;
  if (mis16(qkv) || mis16(k_cache) || mis16(v_cache)) return hipErrorInvalidValue;
  if (H > 65535 || B > 65535) return hipErrorInvalidValue;
  if (len_bound > L_max) len_bound = L_max;
  const int n_chunks = (len_bound + chunk - 1) / chunk;
  DecodeArgs a{static_cast<const uint16_t*>(qkv), static_cast<uint16_t*>(k_cache),
               static_cast<uint16_t*>(v_cache), static_cast<const int*>(length),
               static_cast<float*>(ws), static_cast<uint16_t*>(out), ld, ldo, B, H, L_max, chunk,
               n_chunks, fused ? 1 : 0, scale * 1.4426950408889634f};
  const dim3 gs(n_chunks, H, B), gc(H, B);
  if (D == 64) {
    hipLaunchKernelGGL(attn_decode_split_kernel<64>, gs, dim3(kDecThreads), 0, stream, a);
    hipLaunchKernelGGL(attn_decode_combine_kernel<64>, gc, dim3(64), 0, stream, a);
  } else {
    hipLaunchKernelGGL(attn_decode_split_kernel<128>, gs, dim3(kDecThreads), 0, stream, a);
    hipLaunchKernelGGL(attn_decode_combine_kernel<128>, gc, dim3(128), 0, stream, a);
  }
  return hipGetLastError();
}
