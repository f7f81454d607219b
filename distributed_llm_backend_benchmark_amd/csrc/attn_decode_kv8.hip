// Single-query (decode) attention over an FP8 (OCP e4m3fn) KV cache, gfx950 (MI355X, CDNA4).
//
// Cache layout, per layer and rank: k_cache / v_cache [B, H, L_max, D] e4m3fn bytes, contiguous,
// and k_scale / v_scale [B, H, L_max] fp32: one scale per cached row of D values,
// row ~= float(code) * scale. A row is quantised exactly as gemm_fp8.hip's row quantiser does
// (ops.fp8): amax == 0 -> scale 1, bytes 0; otherwise inv = 448 / amax and scale = amax / 448
// (IEEE fp32 divisions) and code = cvt_pk_fp8_f32(float(x) * inv), round to nearest even. A row
// costs D + 4 bytes against the 2 D of the bf16 cache (attn_decode.hip). `length` is the ONE
// device int32 of that file, with the same meaning; every kernel reads it from device memory.
//
//   kv_append_fp8_kernel          K / V rows of a fused qkv [B, T, 3, H, D] bf16 -> codes and
//                                 scales at cache positions [length, length + T). One row lives
//                                 in D / 8 lanes: a 16-byte load per lane, amax by shuffles, one
//                                 convert pass, an 8-byte store of codes per lane.
//   attn_decode_fp8_split_kernel  grid (n_chunks, H, B), the structure of attn_decode_split_kernel:
//                                 16 bytes per lane are 16 codes, so D / 16 lanes per key. Codes
//                                 go from global memory straight into VGPRs and are widened there
//                                 (v_cvt_pk_f32_fp8, exact); the dot product runs on the raw
//                                 codes, the key's scale is folded into the score
//                                 (s = dot * k_scale * scale_log2) and the value's into the
//                                 weight (o += (p * v_scale) * code, l += p). Online softmax per
//                                 slot, fixed-order merges, fp32 partials (m, l, o[D]) to the
//                                 workspace. No atomics, no tickets: bit-identical run to run.
//   attn_decode_fp8_combine_kernel  the twin of attn_decode_combine_kernel (same arithmetic in the
//                                 same order), so attn_decode.hip stays as it is.
//
// `fused` = 1: the chunk that owns position `length` quantises the token's K / V from `qkv`,
// stores codes + scales and attends to those codes, so the step's result is attention over the
// cache contents after the append, exactly; 0: the caller appended first (dlbb_kv_append_fp8).
#include "common.h"

namespace dlbb {

namespace {

constexpr int kKv8Threads = 256;
constexpr int kKv8Unroll = 4;          // keys in flight per slot (8 x 16 B loads + 8 scales per lane)
constexpr float kKv8NegBig = -1.0e30f; // "no key yet": finite, so no inf - inf in the merges
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

struct KvAppend8Args {
  const uint16_t* qkv;   // [B, T, 3, H, D], token row stride ld
  uint8_t* k_cache;      // [B, H, L_max, D] e4m3fn
  uint8_t* v_cache;
  float* k_scale;        // [B, H, L_max]
  float* v_scale;
  const int* length;
  int64_t ld;
  int B, T, H, L_max;
};

// a row (b, t, k|v, h) of D bf16 per group of D / 8 lanes; uniform trip count over the grid, so
// every lane of a group is active in the shuffles
template <int D>
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(KvAppend8Args a) {
  constexpr int LG = D / 8;                                 // lanes per row
  const int len = *a.length;
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
    const int64_t pos = static_cast<int64_t>(len) + t;
    if (!live || len < 0 || pos >= a.L_max) continue;       // device-side guard: never past the cache
    const int64_t dst = (static_cast<int64_t>(b) * a.H + h) * a.L_max + pos;
    const u32x2 code{f32x4_to_e4m3(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv),
                     f32x4_to_e4m3(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv)};
    *reinterpret_cast<u32x2*>((kv ? a.v_cache : a.k_cache) + dst * D + piece * 8) = code;
    if (piece == 0) (kv ? a.v_scale : a.k_scale)[dst] = scale;
  }
}

struct DecodeKv8Args {
  const uint16_t* qkv;   // [B, 1, 3, H, D], batch row stride ld
  uint8_t* k_cache;      // [B, H, L_max, D] e4m3fn
  uint8_t* v_cache;
  float* k_scale;        // [B, H, L_max]
  float* v_scale;
  const int* length;
  float* ws;             // [B, H, n_chunks, D + 2]: m, l, o[D]
  uint16_t* out;         // [B, 1, H, D], batch row stride ldo
  int64_t ld, ldo;
  int B, H, L_max, chunk, n_chunks, fused;
  float scale_log2;
};

// keys the step attends (and whether the new token has a cache slot): uniform, from device memory
__device__ __forceinline__ int decode_keys(const DecodeKv8Args& a, int& len, bool& room) {
  len = *a.length;
  if (len < 0) len = 0;
  room = len < a.L_max;
  return room ? len + 1 : a.L_max;
}

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

template <int D>
__global__ __launch_bounds__(kKv8Threads) void attn_decode_fp8_split_kernel(DecodeKv8Args a) {
  constexpr int LPK = D / 16;                // lanes per key (16 codes = 16 B each)
  constexpr int NS = kKv8Threads / LPK;      // key slots per workgroup
  constexpr int U = kKv8Unroll;
  __shared__ float red[kKv8Threads / kWave][D + 2];

  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  int len;
  bool room;
  const int L = decode_keys(a, len, room);
  const int k0 = c * a.chunk;
  if (k0 >= L) return;                       // dead chunk: no K / V read, no partial written
  const int k1 = min(k0 + a.chunk, L);
  const int tid = threadIdx.x, sub = tid % LPK, slot = tid / LPK;
  // position whose K / V come from qkv (and are quantised and stored to the cache here); -1: none
  const int newpos = (a.fused && room) ? len : -1;

  const uint16_t* row = a.qkv + static_cast<int64_t>(b) * a.ld + h * D + sub * 16;
  float q[16];
  {
    const u16x8 q0 = *reinterpret_cast<const u16x8*>(row);
    const u16x8 q1 = *reinterpret_cast<const u16x8*>(row + 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      q[j] = bf16_to_f32(q0[j]);
      q[8 + j] = bf16_to_f32(q1[j]);
    }
  }
  const int64_t rows = (static_cast<int64_t>(b) * a.H + h) * a.L_max;
  uint8_t* kc = a.k_cache + rows * D + sub * 16;
  uint8_t* vc = a.v_cache + rows * D + sub * 16;
  float* ksc = a.k_scale + rows;
  float* vsc = a.v_scale + rows;

  // the append, by the chunk owning `length` (workgroup-uniform): every slot holds the token's
  // codes and scales, slot 0 stores them
  u32x4 nk{0, 0, 0, 0}, nv{0, 0, 0, 0};
  float nks = 1.f, nvs = 1.f;
  if (newpos >= k0 && newpos < k1) {
    quant_row16<LPK>(row + a.H * D, nk, nks);
    quant_row16<LPK>(row + 2 * a.H * D, nv, nvs);
    if (slot == 0) {
      *reinterpret_cast<u32x4*>(kc + static_cast<int64_t>(newpos) * D) = nk;
      *reinterpret_cast<u32x4*>(vc + static_cast<int64_t>(newpos) * D) = nv;
      if (sub == 0) {
        ksc[newpos] = nks;
        vsc[newpos] = nvs;
      }
    }
  }

  float m = kKv8NegBig, l = 0.f, o[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) o[j] = 0.f;

  for (int it = k0; it < k1; it += NS * U) {       // uniform trip count over the workgroup
    u32x4 kr[U], vr[U];
    float ks[U], vs[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = it + u * NS + slot;
      ok[u] = key < k1;
      const int kk = ok[u] ? key : k1 - 1;         // masked slots re-read a live row
      // row `newpos` is taken from the registers, never from what the loads below return for it
      // (slot 0's stores may or may not have landed): the loads stay in bounds, kk < L <= L_max
      const bool fresh = kk == newpos;
      const u32x4 kl = *reinterpret_cast<const u32x4*>(kc + static_cast<int64_t>(kk) * D);
      const u32x4 vl = *reinterpret_cast<const u32x4*>(vc + static_cast<int64_t>(kk) * D);
      const float ksl = ksc[kk], vsl = vsc[kk];
      kr[u] = fresh ? nk : kl;
      vr[u] = fresh ? nv : vl;
      ks[u] = fresh ? nks : ksl;
      vs[u] = fresh ? nvs : vsl;
    }
    float s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[16];
      e4m3x16_to_f32(kr[u], kf);
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) d = __builtin_fmaf(q[j], kf[j], d);
#pragma unroll
      for (int off = 1; off < LPK; off <<= 1) d += __shfl_xor(d, off, 64);
      s[u] = ok[u] ? d * ks[u] * a.scale_log2 : kKv8NegBig;
    }
    float mn = m;
#pragma unroll
    for (int u = 0; u < U; ++u) mn = fmaxf(mn, s[u]);
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    l *= alpha;
#pragma unroll
    for (int j = 0; j < 16; ++j) o[j] *= alpha;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = ok[u] ? __builtin_amdgcn_exp2f(s[u] - mn) : 0.f;
      float vf[16];
      e4m3x16_to_f32(vr[u], vf);
      l += p;
      const float pv = p * vs[u];
#pragma unroll
      for (int j = 0; j < 16; ++j) o[j] = __builtin_fmaf(pv, vf[j], o[j]);
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
    for (int j = 0; j < 16; ++j) {
      const float o2 = __shfl_xor(o[j], off, 64);
      const float oa = lo ? o[j] * f1 : o2 * f2, ob = lo ? o2 * f2 : o[j] * f1;
      o[j] = oa + ob;
    }
    m = mn;
  }
  const int lane = tid & (kWave - 1), w = tid / kWave;
  if (lane < LPK) {
#pragma unroll
    for (int j = 0; j < 16; ++j) red[w][sub * 16 + j] = o[j];
    if (sub == 0) {
      red[w][D] = m;
      red[w][D + 1] = l;
    }
  }
  __syncthreads();
  if (tid < D) {                                   // the 4 waves, in wave order
    float mw = red[0][D];
#pragma unroll
    for (int i = 1; i < kKv8Threads / kWave; ++i) mw = fmaxf(mw, red[i][D]);
    float lw = 0.f, ow = 0.f;
#pragma unroll
    for (int i = 0; i < kKv8Threads / kWave; ++i) {
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
__global__ __launch_bounds__(D) void attn_decode_fp8_combine_kernel(DecodeKv8Args a) {
  const int h = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  int len;
  bool room;
  const int L = decode_keys(a, len, room);
  const int live = min((L + a.chunk - 1) / a.chunk, a.n_chunks);
  const float* p = a.ws + (static_cast<int64_t>(b) * a.H + h) * a.n_chunks * (D + 2);
  float mx = kKv8NegBig;
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

}  // namespace

}  // namespace dlbb

using namespace dlbb;

// qkv: [B, T, 3, H, D] bf16 (token row stride ld elements); k_cache / v_cache: [B, H, L_max, D]
// e4m3fn contiguous; k_scale / v_scale: [B, H, L_max] fp32 contiguous; length: device int32. Rows
// K / V of every token are quantised to cache positions [*length, *length + T); positions >= L_max
// (and every position when *length < 0) are dropped on the device.
DLBB_API int dlbb_kv_append_fp8(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                void* k_scale, void* v_scale, const void* length, int B, int T,
                                int H, int D, int L_max, hipStream_t stream) {
  if (B <= 0 || T <= 0 || H <= 0) return hipSuccess;
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  if (L_max <= 0 || ld % 8 || ld < 3 * H * D || !length) return hipErrorInvalidValue;
  if (!k_cache || !v_cache || !k_scale || !v_scale) return hipErrorInvalidValue;
  if (mis(qkv, 16) || mis(k_cache, 16) || mis(v_cache, 16) || mis(k_scale, 4) || mis(v_scale, 4))
    return hipErrorInvalidValue;
  KvAppend8Args a{static_cast<const uint16_t*>(qkv), static_cast<uint8_t*>(k_cache),
                  static_cast<uint8_t*>(v_cache), static_cast<float*>(k_scale),
                  static_cast<float*>(v_scale), static_cast<const int*>(length), ld, B, T, H,
                  L_max};
  const int64_t lanes = static_cast<int64_t>(B) * T * 2 * H * (D / 8);
  const dim3 grid(stream_grid(lanes, 256));
  if (D == 64)
    hipLaunchKernelGGL(kv_append_fp8_kernel<64>, grid, dim3(256), 0, stream, a);
  else
    hipLaunchKernelGGL(kv_append_fp8_kernel<128>, grid, dim3(256), 0, stream, a);
  return hipGetLastError();
}

// One decode step of attention over the FP8 cache: qkv [B, 1, 3, H, D] bf16 (batch row stride
// ld), the cache as above, out [B, 1, H, D] bf16 (batch row stride ldo). Attends over *length + 1
// keys; with fused != 0 the new token's K / V are quantised from qkv and stored at position
// *length by the same launch (and attended to in their quantised form), else the caller has
// appended them already. ws: fp32 [B, H, n_chunks, D + 2], n_chunks = ceil(min(len_bound, L_max)
// / chunk); len_bound is the host's upper bound of *length + 1.
DLBB_API int dlbb_attn_decode_fp8(const void* qkv, int64_t ld, void* k_cache, void* v_cache,
                                  void* k_scale, void* v_scale, const void* length, void* ws,
                                  void* out, int64_t ldo, int B, int H, int D, int L_max,
                                  int len_bound, int chunk, int fused, float scale,
                                  hipStream_t stream) {
  if (B <= 0 || H <= 0) return hipSuccess;
  if (D != 64 && D != 128) return hipErrorInvalidValue;
  if (L_max <= 0 || chunk <= 0 || len_bound <= 0 || !length || !ws) return hipErrorInvalidValue;
  if (ld % 8 || ld < 3 * H * D || ldo < H * D) return hipErrorInvalidValue;
  if (!k_cache || !v_cache || !k_scale || !v_scale || !out) return hipErrorInvalidValue;
  if (mis(qkv, 16) || mis(k_cache, 16) || mis(v_cache, 16) || mis(k_scale, 4) || mis(v_scale, 4))
    return hipErrorInvalidValue;
  if (H > 65535 || B > 65535) return hipErrorInvalidValue;
  if (len_bound > L_max) len_bound = L_max;
  const int n_chunks = (len_bound + chunk - 1) / chunk;
  DecodeKv8Args a{static_cast<const uint16_t*>(qkv), static_cast<uint8_t*>(k_cache),
                  static_cast<uint8_t*>(v_cache), static_cast<float*>(k_scale),
                  static_cast<float*>(v_scale), static_cast<const int*>(length),
                  static_cast<float*>(ws), static_cast<uint16_t*>(out), ld, ldo, B, H, L_max,
                  chunk, n_chunks, fused ? 1 : 0, scale * 1.4426950408889634f};
  const dim3 gs(n_chunks, H, B), gc(H, B);
  if (D == 64) {
    hipLaunchKernelGGL(attn_decode_fp8_split_kernel<64>, gs, dim3(kKv8Threads), 0, stream, a);
    hipLaunchKernelGGL(attn_decode_fp8_combine_kernel<64>, gc, dim3(64), 0, stream, a);
  } else {
    hipLaunchKernelGGL(attn_decode_fp8_split_kernel<128>, gs, dim3(kKv8Threads), 0, stream, a);
    hipLaunchKernelGGL(attn_decode_fp8_combine_kernel<128>, gc, dim3(128), 0, stream, a);
  }
  return hipGetLastError();
}
