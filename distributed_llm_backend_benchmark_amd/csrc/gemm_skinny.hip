// Skinny-M weight-streaming GEMM for the decode step's linears, gfx950: bf16 weights,
// weight-only FP8 (W8A16: e4m3fn weights, bf16 activations) or weight-only MXFP4 (W4A16: e2m1
// codes with one e8m0 scale per block of 32 k, bf16 activations).
//
//   out[M,N] = epilogue( x[M,K] · W[N,K]^T ),  1 <= M <= 16, N % 16 == 0, K % 64 == 0
//   (W4: K % 128 == 0)
//   epilogue: (* wscale[N], W8 only) -> (+ bias[N]) -> (GELU erf | GELU tanh) ->
//   (+ residual[M,N]) -> bf16 | fp32 store
//   (the meaning of dlbb_gemm_bf16_nt_v without the pre-activation output, which is training
//   only). W8: Wq holds e4m3fn bytes with one fp32 scale per output row
//   (ops.fp8.quantize_weight); the row scale multiplies the fp32 accumulator ahead of the bias,
//   the order of the FP8 GEMM (gemm_fp8.hip). W4: Wq holds two e2m1 codes per byte (element 2j in
//   the low nibble of byte j) and S one e8m0 byte per 32 consecutive k of a row, value = code *
//   2^(S - 127) (ops.mxfp4.quantize_mxfp4); there is no row scale and no scale step in the
//   epilogue.
//
// At M = batch rows the 256² / 128² tiles of gemm.hip are > 90 % padding and the step is a pure
// stream of W (the W8 form streams half the bytes). This kernel reads W exactly once, straight
// from global memory into VGPRs (16 B per lane, a batch of loads in flight, then counted waits)
// — no LDS staging: nothing is shared between waves, so the LDS round trip would be pure
// overhead.
//
//   * A workgroup owns 16 rows of W (one column tile of out); its `kw` waves split K into
//     contiguous ranges of 64-element units.
//   * v_mfma_f32_16x16x32_bf16 with A = W (row = lane & 15) and B = x^T (column = lane & 15 = the
//     row m of x), so lane l ends with out[m = l & 15][n0 + 4 (l >> 4) + 0..3]: four contiguous
//     outputs per lane, one 16-byte (fp32) or 8-byte (bf16) store.
//   * The dot product does not care about the order of k: within a unit lane group q = l >> 4
//     reads the 16 contiguous elements [16 q, 16 q + 16) of its W row and the same elements of
//     its x row (two 16-B loads), so both MFMAs of the unit see one k-permutation on both
//     operands.
//   * Lanes whose x row is >= M read row 0 instead (always valid; the same addresses as the
//     lanes of row 0, so no extra traffic). Their MFMA columns hold garbage that no other
//     column depends on, and they store nothing: rows >= M of x are never read, rows >= M of
//     out never written.
//   * The waves' 16 x 16 fp32 partial blocks are summed through LDS by wave 0 in wave order — a
//     fixed order, so results are bit-identical from run to run. No atomics, no device
//     workspace, no dependence on any other workgroup: safe beside communication kernels and
//     inside graph capture.
//
// The operand path differs:
//   * bf16: a lane's 16 elements of W are two 16-B loads, fed straight to the two MFMAs.
//   * W8: they are one 16-B load; its low and high 8 bytes are widened to two bf16x8 operands with
//     v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 — one instruction per packed pair, 8 per unit (the
//     v_cvt_pk_f32_fp8 route needs 8 converts plus 8 v_perm_b32 to pack the high half-words).
//     e4m3fn has 3 mantissa bits and its exponent range lies inside bf16's, so the conversion is
//     exact (subnormals included). Each operand feeds one MFMA against the matching half of x.
//   * W4: a lane's 16-B load is 32 codes = exactly one MX block, so a unit is 128 k here: lane
//     group q reads the block [32 q, 32 q + 32) of its row, one scale byte, and the same 32
//     elements of its x row (four 16-B loads). v_cvt_scalef32_pk_bf16_fp4 widens one byte (low
//     nibble first) to two bf16 and multiplies by the block scale — the float whose bits are
//     S << 23 — in one instruction, 16 per unit; dword j of the load becomes the operand of MFMA j
//     against x elements [32 q + 8 j, 32 q + 8 j + 8), the same k order on both sides. The
//     quantiser emits S in [2, 252], so every product code * 2^(S - 127) is a normal (or zero)
//     bf16 and the conversion is exact.
#include "common.h"

namespace dlbb {

namespace {

constexpr int SK_EPI_BIAS = 1, SK_EPI_GELU_ERF = 2, SK_EPI_GELU_TANH = 4, SK_EPI_RESIDUAL = 8;
// elements of W's storage type per unit and per row: 64 bf16, 64 e4m3 bytes, or 64 bytes of
// e2m1 codes. A lane owns 16 of them: 16 k and two MFMAs (bf16, W8), or 32 k and four (W4)
constexpr int kSkUnit = 64;
constexpr int kSkMaxWaves = 16;    // waves per workgroup (1024 threads)
constexpr int kSkWavesPerCU = 16;  // the plan's target of resident waves per CU over the whole grid
// units per batch of loads. bf16: 8 W + 8 x loads of 16 B in flight. W8: 4 W + 8 x loads ahead
// of the first wait, 48 VGPRs of operands, 72 in all; measured against 2, 3, 5, 6 and 8 units on
// the TP-7B shapes (docs/PERFORMANCE.md): 2 and 3 are no faster, 5 / 6 / 8 up to 14 / 6 / 23 %
// slower at world 1 — the wave ranges there are 4 or 16 units or 10-11, so deeper batches leave
// more to the tail batch, and their registers cost residency. W4 batches 2 units (WMxfp4 below)
constexpr int kSkUnroll = 4;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16v2 __attribute__((ext_vector_type(2)));

struct SkinnyArgs {
  const uint16_t* x;
  const void* w;                   // bf16, e4m3fn bytes or e2m1 code pairs
  void* out;
  const uint16_t* bias;
  const uint16_t* residual;
  int64_t lda, ldw, ldr;
  int M, N, K;
  int epi;
  int out_f32;
  int kw;                          // waves per workgroup = K-split inside the workgroup
  int uq, ur;                      // units / kw, units % kw: wave w owns uq (+1 if w < ur) units
  const void* wscale;              // W8: fp32 [N]; W4: e8m0 bytes [N, K / 32]; bf16: null
};

__device__ __forceinline__ bf16x8 ld16(const uint16_t* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}

// 8 e4m3fn bytes (two dwords) -> 8 bf16 in byte order, exactly
__device__ __forceinline__ bf16x8 widen8(uint32_t a, uint32_t b) {
  struct { bf16v2 v[4]; } p;
  p.v[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, false);
  p.v[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(a, 1.0f, true);
  p.v[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, false);
  p.v[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(b, 1.0f, true);
  return __builtin_bit_cast(bf16x8, p);
}

// 8 e2m1 codes (one dword, element 2j in the low nibble of byte j) times the block scale `s`
// -> 8 bf16 in element order
__device__ __forceinline__ bf16x8 widen8_fp4(uint32_t a, float s) {
  struct { bf16v2 v[4]; } p;
  p.v[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, s, 0);
  p.v[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, s, 1);
  p.v[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, s, 2);
  p.v[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(a, s, 3);
  return __builtin_bit_cast(bf16x8, p);
}

// What differs between the weight formats: a lane's 16 storage elements of W per unit (their
// load and the MFMA operands made of them: kOps of them, against 8 kOps elements of x), the
// scales, the plan's floor and the shape of the tail.
struct WBf16 {
  using Elem = uint16_t;
  struct Frag { bf16x8 lo, hi; };
  static constexpr int kOps = 2;           // MFMAs per unit; a unit is 32 kOps elements of k
  static constexpr int kPack = 1;          // k elements per Elem
  static constexpr int kScaleAlign = 0;    // alignment of the scales; 0: the format has none
  static constexpr bool kScaled = false;   // one fp32 scale per row, applied in the epilogue
  static constexpr int kMinUnits = 2;      // a wave's K-range is at least this many units
  static constexpr int kUnroll = kSkUnroll;  // units per batch of loads
  static constexpr bool kBatchedTail = false;
  static __device__ __forceinline__ Frag load(const Elem* p, const uint8_t*) {
    return {ld16(p), ld16(p + 8)};
  }
  static __device__ __forceinline__ bf16x8 lo(const Frag& w) { return w.lo; }
  static __device__ __forceinline__ bf16x8 hi(const Frag& w) { return w.hi; }
};
struct WE4m3 {
  using Elem = uint8_t;
  using Frag = u32x4;
  static constexpr int kOps = 2;
  static constexpr int kPack = 1;
  static constexpr int kScaleAlign = 16;
  static constexpr bool kScaled = true;
  // A unit is 1 KiB of W per wave here, half the bf16 kernel's, so its minimum of 2 units would
  // leave a wave 2 KiB to stream — half a batch of loads, all latency. 4 units keep the bf16
  // kernel's 4 KiB floor per wave and are one full batch (2 measured no faster on any row, 5 %
  // slower at N = 4096, K = 512).
  static constexpr int kMinUnits = 4;
  static constexpr int kUnroll = kSkUnroll;
  static constexpr bool kBatchedTail = true;
  static __device__ __forceinline__ Frag load(const Elem* p, const uint8_t*) {
    return *reinterpret_cast<const Frag*>(p);
  }
  static __device__ __forceinline__ bf16x8 lo(const Frag& w) { return widen8(w[0], w[1]); }
  static __device__ __forceinline__ bf16x8 hi(const Frag& w) { return widen8(w[2], w[3]); }
};
struct WMxfp4 {
  using Elem = uint8_t;                    // two e2m1 codes
  struct Frag { u32x4 c; uint32_t s; };    // a lane's MX block: 32 codes and their e8m0 byte
  static constexpr int kOps = 4;
  static constexpr int kPack = 2;
  static constexpr int kScaleAlign = 4;
  static constexpr bool kScaled = false;   // the block scale goes into the convert
  // a unit is 1 KiB of W per wave, as a W8 unit is: its floor and its tail (a floor of 2 measured
  // no faster on any world-1 shape, one of 8 5 % slower at N = K = 4096)
  static constexpr int kMinUnits = 4;
  // 2 units per batch: 2 W + 2 scale + 8 x loads in flight, 64 VGPRs. 4 units (20 loads, 121
  // VGPRs) measured 21 % slower on the world-1 QKV shape and 1-3 % slower on the other three,
  // 3 units 14 % slower at N = K = 4096, 1 unit 2-4 % slower on up and down
  // (docs/PERFORMANCE.md)
  static constexpr int kUnroll = 2;
  static constexpr bool kBatchedTail = true;
  static __device__ __forceinline__ Frag load(const Elem* p, const uint8_t* s) {
    return {*reinterpret_cast<const u32x4*>(p), *s};
  }
  template <int J>
  static __device__ __forceinline__ bf16x8 op(const Frag& w) {
    return widen8_fp4(w.c[J], __builtin_bit_cast(float, w.s << 23));
  }
};

template <typename Fmt>
__device__ __forceinline__ void unit_mfma(const typename Fmt::Frag& w,
                                          const bf16x8 (&x)[Fmt::kOps], f32x4& acc0,
                                          f32x4& acc1) {
  if constexpr (Fmt::kOps == 2) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Fmt::lo(w), x[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Fmt::hi(w), x[1], acc1, 0, 0, 0);
  } else {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Fmt::template op<0>(w), x[0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Fmt::template op<1>(w), x[1], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Fmt::template op<2>(w), x[2], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Fmt::template op<3>(w), x[3], acc1, 0, 0, 0);
  }
}

// a lane's 8 kOps elements of x for one unit
template <typename Fmt>
__device__ __forceinline__ void load_x(const uint16_t* p, bf16x8 (&x)[Fmt::kOps]) {
#pragma unroll
  for (int j = 0; j < Fmt::kOps; ++j) x[j] = ld16(p + 8 * j);
}

template <typename Fmt>
__global__ __launch_bounds__(kSkMaxWaves * 64) void gemm_nt_skinny_kernel(SkinnyArgs a) {
  using Frag = typename Fmt::Frag;
  constexpr int kOps = Fmt::kOps;
  constexpr int kXUnit = 32 * kOps;             // k elements per unit
  constexpr int kUnroll = Fmt::kUnroll;
  extern __shared__ f32x4 sk_part[];            // [kw][64 lanes] partial blocks
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * 16;
  // wave's contiguous unit range (balanced; every wave has >= Fmt::kMinUnits by the plan)
  const int u0 = wave * a.uq + (wave < a.ur ? wave : a.ur);
  const int u1 = u0 + a.uq + (wave < a.ur ? 1 : 0);
  const int xr = fr < a.M ? fr : 0;
  const typename Fmt::Elem* wp = static_cast<const typename Fmt::Elem*>(a.w) +
                                 static_cast<int64_t>(n0 + fr) * a.ldw + fq * 16;
  const uint16_t* xp = a.x + static_cast<int64_t>(xr) * a.lda + fq * (8 * kOps);
  // W4: the lane's block scale of unit u is byte 4 u of sp; null otherwise and never read
  const uint8_t* sp = nullptr;
  if constexpr (Fmt::kScaleAlign && !Fmt::kScaled)
    sp = static_cast<const uint8_t*>(a.wscale) + static_cast<int64_t>(n0 + fr) * (a.K / 32) + fq;

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int u = u0;
  for (; u + kUnroll <= u1; u += kUnroll) {
    Frag wf[kUnroll];
    bf16x8 xf[kUnroll][kOps];
#pragma unroll
    for (int i = 0; i < kUnroll; ++i)
      wf[i] = Fmt::load(wp + (u + i) * kSkUnit, sp + (u + i) * 4);
#pragma unroll
    for (int i = 0; i < kUnroll; ++i) load_x<Fmt>(xp + (u + i) * kXUnit, xf[i]);
    __builtin_amdgcn_sched_barrier(0);          // the whole batch is in flight before any wait
#pragma unroll
    for (int i = 0; i < kUnroll; ++i) unit_mfma<Fmt>(wf[i], xf[i], acc0, acc1);
  }
  if constexpr (Fmt::kBatchedTail) {
    if (u < u1) {
      // the last 1 .. kUnroll - 1 units as one batch too: a slot past the range loads the
      // range's last unit again (in bounds, the same addresses) and its MFMAs are skipped
      const int rem = u1 - u;                   // wave-uniform
      Frag wf[kUnroll - 1];
      bf16x8 xf[kUnroll - 1][kOps];
#pragma unroll
      for (int i = 0; i < kUnroll - 1; ++i) {
        const int ui = u + (i < rem ? i : rem - 1);
        wf[i] = Fmt::load(wp + ui * kSkUnit, sp + ui * 4);
        load_x<Fmt>(xp + ui * kXUnit, xf[i]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < kUnroll - 1; ++i) {
        if (i < rem) unit_mfma<Fmt>(wf[i], xf[i], acc0, acc1);
      }
    }
  } else {
    for (; u < u1; ++u) {                       // unit by unit
      const Frag w = Fmt::load(wp + u * kSkUnit, sp + u * 4);
      bf16x8 x[kOps];
      load_x<Fmt>(xp + u * kXUnit, x);
      unit_mfma<Fmt>(w, x, acc0, acc1);
    }
  }
  f32x4 v = acc0 + acc1;

  if (a.kw > 1) {                               // wave-uniform
    sk_part[wave * 64 + lane] = v;
    __syncthreads();
    if (wave != 0) return;
    v = sk_part[lane];
    for (int s = 1; s < a.kw; ++s) v += sk_part[s * 64 + lane];   // fixed order
  }
  if (fr >= a.M) return;                        // padding columns of the MFMA: nothing stored

  const int n = n0 + fq * 4;
  const int epi = a.epi;
  if constexpr (Fmt::kScaled)
    v *= *reinterpret_cast<const f32x4*>(static_cast<const float*>(a.wscale) + n);
  if (epi & SK_EPI_BIAS) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += bf16_to_f32(a.bias[n + r]);
  }
  if (epi & SK_EPI_GELU_ERF) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
  } else if (epi & SK_EPI_GELU_TANH) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = gelu_tanh(v[r]);
  }
  if (epi & SK_EPI_RESIDUAL) {
    const uint16_t* rp = a.residual + static_cast<int64_t>(fr) * a.ldr + n;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += bf16_to_f32(rp[r]);
  }
  const int64_t o = static_cast<int64_t>(fr) * a.N + n;
  if (a.out_f32) {
    *reinterpret_cast<f32x4*>(static_cast<float*>(a.out) + o) = v;
  } else {
    u16x4 b;
#pragma unroll
    for (int r = 0; r < 4; ++r) b[r] = f32_to_bf16(v[r]);
    *reinterpret_cast<u16x4*>(static_cast<uint16_t*>(a.out) + o) = b;
  }
}

// out = {grid (workgroups, one per 16 rows of W), K-split inside a workgroup (waves), K-split
// across workgroups (always 1: this kernel has no cross-workgroup combine), workspace bytes
// (always 0)}; returns 0 outside the contract. The in-workgroup split aims at ~kSkWavesPerCU
// waves per CU over the whole grid with at least `min_units` units of `unit_k` elements per wave.
int skinny_plan(int64_t M, int64_t N, int64_t K, int ncu, int min_units, int unit_k,
                int64_t* out) {
  if (M < 1 || M > 16 || N <= 0 || N % 16 || K <= 0 || K % unit_k || ncu <= 0) return 0;
  if (N / 16 > 0x7fffffffLL || K > 0x7fffffffLL) return 0;
  const int64_t tiles = N / 16, units = K / unit_k;
  int64_t kw = (static_cast<int64_t>(ncu) * kSkWavesPerCU + tiles - 1) / tiles;
  if (kw > units / min_units) kw = units / min_units;
  if (kw > kSkMaxWaves) kw = kSkMaxWaves;
  if (kw < 1) kw = 1;
  out[0] = tiles;
  out[1] = kw;
  out[2] = 1;
  out[3] = 0;
  return 1;
}

// the contract checks and the launch of the entry points; ldb in storage elements of W
template <typename Fmt>
int skinny_launch(const void* A, int64_t lda, const void* B, int64_t ldb, const void* wscale,
                  void* C, int64_t M, int64_t N, int64_t K, const void* bias,
                  const void* residual, int64_t ldr, int epi, int out_f32, int ncu,
                  hipStream_t stream) {
  constexpr int unit_k = 32 * Fmt::kOps;
  int64_t plan[4];
  if (!skinny_plan(M, N, K, ncu, Fmt::kMinUnits, unit_k, plan)) return hipErrorInvalidValue;
  constexpr int ldb_mult = 16 / static_cast<int>(sizeof(typename Fmt::Elem));   // 16 bytes
  if (!A || !B || !C || lda % 8 || ldb % ldb_mult || lda < K || ldb < K / Fmt::kPack)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) |
       reinterpret_cast<uintptr_t>(C)) & 15)
    return hipErrorInvalidValue;
  if (Fmt::kScaleAlign &&
      (!wscale || (reinterpret_cast<uintptr_t>(wscale) & (Fmt::kScaleAlign - 1))))
    return hipErrorInvalidValue;
  if (epi & ~(SK_EPI_BIAS | SK_EPI_GELU_ERF | SK_EPI_GELU_TANH | SK_EPI_RESIDUAL))
    return hipErrorInvalidValue;
  if ((epi & SK_EPI_GELU_ERF) && (epi & SK_EPI_GELU_TANH)) return hipErrorInvalidValue;
  if ((epi & SK_EPI_BIAS) && !bias) return hipErrorInvalidValue;
  if ((epi & SK_EPI_RESIDUAL) && (!residual || ldr < N)) return hipErrorInvalidValue;
  SkinnyArgs a{static_cast<const uint16_t*>(A), B, C,
               static_cast<const uint16_t*>(bias), static_cast<const uint16_t*>(residual),
               lda, ldb, ldr, static_cast<int>(M), static_cast<int>(N), static_cast<int>(K),
               epi, out_f32, static_cast<int>(plan[1]),
               static_cast<int>((K / unit_k) / plan[1]), static_cast<int>((K / unit_k) % plan[1]),
               wscale};
  const dim3 g(static_cast<unsigned>(plan[0])), b(static_cast<unsigned>(plan[1] * 64));
  const size_t lds = plan[1] > 1 ? static_cast<size_t>(plan[1]) * 64 * sizeof(f32x4) : 0;
  hipLaunchKernelGGL(gemm_nt_skinny_kernel<Fmt>, g, b, lds, stream, a);
  return hipGetLastError();
}

}  // namespace

}  // namespace dlbb

using namespace dlbb;

// Plan of the skinny GEMM for an [M, K] x [N, K]^T shape on `ncu` CUs (skinny_plan above), with
// at least 2 units per wave.
DLBB_API int dlbb_gemm_skinny_plan(int64_t M, int64_t N, int64_t K, int ncu, int64_t* out) {
  return skinny_plan(M, N, K, ncu, WBf16::kMinUnits, 32 * WBf16::kOps, out);
}

// The W8 form's plan: at least 4 units per wave. This kernel stays out of the autotuner.
DLBB_API int dlbb_gemm_w8_skinny_plan(int64_t M, int64_t N, int64_t K, int ncu, int64_t* out) {
  return skinny_plan(M, N, K, ncu, WE4m3::kMinUnits, 32 * WE4m3::kOps, out);
}

// The W4 form's plan: at least 4 units of 128 k per wave. Out of the autotuner too.
DLBB_API int dlbb_gemm_w4_skinny_plan(int64_t M, int64_t N, int64_t K, int ncu, int64_t* out) {
  return skinny_plan(M, N, K, ncu, WMxfp4::kMinUnits, 32 * WMxfp4::kOps, out);
}

// out[M, N] = act(A[M, K] · B[N, K]^T + bias) + residual on the caller's stream; `out` is
// contiguous (row stride N), bf16 or fp32 (out_f32). Outside the contract (1 <= M <= 16,
// N % 16 == 0, K % 64 == 0, lda / ldb multiples of 8 elements and >= K, 16-byte aligned A / B /
// out, epi within bias | GELU | residual with at most one GELU, non-null pointers for what epi
// names) nothing is launched and hipErrorInvalidValue is returned.
DLBB_API int dlbb_gemm_bf16_nt_skinny(const void* A, int64_t lda, const void* B, int64_t ldb,
                                      void* C, int64_t M, int64_t N, int64_t K, const void* bias,
                                      const void* residual, int64_t ldr, int epi, int out_f32,
                                      int ncu, hipStream_t stream) {
  return skinny_launch<WBf16>(A, lda, B, ldb, nullptr, C, M, N, K, bias, residual, ldr, epi,
                              out_f32, ncu, stream);
}

// out[M, N] = act((A[M, K] · Bq[N, K]^T) * wscale[N] + bias) + residual: A bf16, Bq e4m3fn bytes,
// wscale fp32. The contract above, with ldb a multiple of 16 bytes and wscale non-null and
// 16-byte aligned.
DLBB_API int dlbb_gemm_w8_nt_skinny(const void* A, int64_t lda, const void* Bq, int64_t ldb,
                                    const void* wscale, void* C, int64_t M, int64_t N, int64_t K,
                                    const void* bias, const void* residual, int64_t ldr, int epi,
                                    int out_f32, int ncu, hipStream_t stream) {
  return skinny_launch<WE4m3>(A, lda, Bq, ldb, wscale, C, M, N, K, bias, residual, ldr, epi,
                              out_f32, ncu, stream);
}

// out[M, N] = act(A[M, K] · dequant(Bq, scales)[N, K]^T + bias) + residual: A bf16, Bq e2m1 code
// pairs [N, K / 2] with a leading dimension of ldb_bytes, scales e8m0 bytes, contiguous
// [N, K / 32]. The contract of the bf16 form with K % 128 == 0, ldb_bytes a multiple of 16 and
// >= K / 2, and scales non-null and 4-byte aligned.
DLBB_API int dlbb_gemm_w4_nt_skinny(const void* A, int64_t lda, const void* Bq, int64_t ldb_bytes,
                                    const void* scales, void* C, int64_t M, int64_t N, int64_t K,
                                    const void* bias, const void* residual, int64_t ldr, int epi,
                                    int out_f32, int ncu, hipStream_t stream) {
  return skinny_launch<WMxfp4>(A, lda, Bq, ldb_bytes, scales, C, M, N, K, bias, residual, ldr,
                               epi, out_f32, ncu, stream);
}
