// Skinny-M weight-streaming GEMM for the decode step's linears, gfx950: bf16 weights, or
// weight-only FP8 (W8A16: e4m3fn weights, bf16 activations).
//
//   out[M,N] = epilogue( x[M,K] · W[N,K]^T ),  1 <= M <= 16, N % 16 == 0, K % 64 == 0
//   epilogue: (* wscale[N], W8 only) -> (+ bias[N]) -> (GELU erf | GELU tanh) ->
//   (+ residual[M,N]) -> bf16 | fp32 store
//   (the meaning of dlbb_gemm_bf16_nt_v without the pre-activation output, which is training
//   only). W8: Wq holds e4m3fn bytes with one fp32 scale per output row
//   (ops.fp8.quantize_weight); the row scale multiplies the fp32 accumulator ahead of the bias,
//   the order of the FP8 GEMM (gemm_fp8.hip).
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
#include "common.h"

namespace dlbb {

namespace {

constexpr int SK_EPI_BIAS = 1, SK_EPI_GELU_ERF = 2, SK_EPI_GELU_TANH = 4, SK_EPI_RESIDUAL = 8;
constexpr int kSkUnit = 64;        // k elements per unit: two MFMAs, 16 elements per lane per operand
constexpr int kSkMaxWaves = 16;    // waves per workgroup (1024 threads)
constexpr int kSkWavesPerCU = 16;  // the plan's target of resident waves per CU over the whole grid
// units per batch of loads. bf16: 8 W + 8 x loads of 16 B in flight. W8: 4 W + 8 x loads ahead
// of the first wait, 48 VGPRs of operands, 72 in all; measured against 2, 3, 5, 6 and 8 units on
// the TP-7B shapes (docs/PERFORMANCE.md): 2 and 3 are no faster, 5 / 6 / 8 up to 14 / 6 / 23 %
// slower at world 1 — the wave ranges there are 4 or 16 units or 10-11, so deeper batches leave
// more to the tail batch, and their registers cost residency
constexpr int kSkUnroll = 4;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16v2 __attribute__((ext_vector_type(2)));

struct SkinnyArgs {
  const uint16_t* x;
  const void* w;                   // bf16 or e4m3fn bytes
  void* out;
  const uint16_t* bias;
  const uint16_t* residual;
  int64_t lda, ldw, ldr;
  int M, N, K;
  int epi;
  int out_f32;
  int kw;                          // waves per workgroup = K-split inside the workgroup
  int uq, ur;                      // units / kw, units % kw: wave w owns uq (+1 if w < ur) units
  const float* wscale;             // [N]; null for bf16 weights
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

// What differs between the weight formats: a lane's 16 elements of W per unit (their load and
// the two MFMA operands made of them), the row scale, the plan's floor and the shape of the tail.
struct WBf16 {
  using Elem = uint16_t;
  struct Frag { bf16x8 lo, hi; };
  static constexpr bool kScaled = false;
  static constexpr int kMinUnits = 2;      // a wave's K-range is at least this many units
  static constexpr bool kBatchedTail = false;
  static __device__ __forceinline__ Frag load(const Elem* p) { return {ld16(p), ld16(p + 8)}; }
  static __device__ __forceinline__ bf16x8 lo(const Frag& w) { return w.lo; }
  static __device__ __forceinline__ bf16x8 hi(const Frag& w) { return w.hi; }
};
struct WE4m3 {
  using Elem = uint8_t;
  using Frag = u32x4;
  static constexpr bool kScaled = true;
  // A unit is 1 KiB of W per wave here, half the bf16 kernel's, so its minimum of 2 units would
  // leave a wave 2 KiB to stream — half a batch of loads, all latency. 4 units keep the bf16
  // kernel's 4 KiB floor per wave and are one full batch (2 measured no faster on any row, 5 %
  // slower at N = 4096, K = 512).
  static constexpr int kMinUnits = 4;
  static constexpr bool kBatchedTail = true;
  static __device__ __forceinline__ Frag load(const Elem* p) {
    return *reinterpret_cast<const Frag*>(p);
  }
  static __device__ __forceinline__ bf16x8 lo(const Frag& w) { return widen8(w[0], w[1]); }
  static __device__ __forceinline__ bf16x8 hi(const Frag& w) { return widen8(w[2], w[3]); }
};

template <typename Fmt>
__device__ __forceinline__ void unit_mfma(const typename Fmt::Frag& w, const bf16x8& x0,
                                          const bf16x8& x1, f32x4& acc0, f32x4& acc1) {
  acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Fmt::lo(w), x0, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Fmt::hi(w), x1, acc1, 0, 0, 0);
}

template <typename Fmt>
__global__ __launch_bounds__(kSkMaxWaves * 64) void gemm_nt_skinny_kernel(SkinnyArgs a) {
  using Frag = typename Fmt::Frag;
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
  const uint16_t* xp = a.x + static_cast<int64_t>(xr) * a.lda + fq * 16;

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int u = u0;
  for (; u + kSkUnroll <= u1; u += kSkUnroll) {
    Frag wf[kSkUnroll];
    bf16x8 xf[kSkUnroll][2];
#pragma unroll
    for (int i = 0; i < kSkUnroll; ++i) wf[i] = Fmt::load(wp + (u + i) * kSkUnit);
#pragma unroll
    for (int i = 0; i < kSkUnroll; ++i) {
      xf[i][0] = ld16(xp + (u + i) * kSkUnit);
      xf[i][1] = ld16(xp + (u + i) * kSkUnit + 8);
    }
    __builtin_amdgcn_sched_barrier(0);          // the whole batch is in flight before any wait
#pragma unroll
    for (int i = 0; i < kSkUnroll; ++i) unit_mfma<Fmt>(wf[i], xf[i][0], xf[i][1], acc0, acc1);
  }
  if constexpr (Fmt::kBatchedTail) {
    if (u < u1) {
      // the last 1 .. kSkUnroll - 1 units as one batch too: a slot past the range loads the
      // range's last unit again (in bounds, the same addresses) and its MFMAs are skipped
      const int rem = u1 - u;                   // wave-uniform
      Frag wf[kSkUnroll - 1];
      bf16x8 xf[kSkUnroll - 1][2];
#pragma unroll
      for (int i = 0; i < kSkUnroll - 1; ++i) {
        const int ui = u + (i < rem ? i : rem - 1);
        wf[i] = Fmt::load(wp + ui * kSkUnit);
        xf[i][0] = ld16(xp + ui * kSkUnit);
        xf[i][1] = ld16(xp + ui * kSkUnit + 8);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < kSkUnroll - 1; ++i) {
        if (i < rem) unit_mfma<Fmt>(wf[i], xf[i][0], xf[i][1], acc0, acc1);
      }
    }
  } else {
    for (; u < u1; ++u) {                       // unit by unit
      const Frag w = Fmt::load(wp + u * kSkUnit);
      const bf16x8 x0 = ld16(xp + u * kSkUnit), x1 = ld16(xp + u * kSkUnit + 8);
      unit_mfma<Fmt>(w, x0, x1, acc0, acc1);
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
  if constexpr (Fmt::kScaled) v *= *reinterpret_cast<const f32x4*>(a.wscale + n);
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
// waves per CU over the whole grid with at least `min_units` 64-element units per wave.
int skinny_plan(int64_t M, int64_t N, int64_t K, int ncu, int min_units, int64_t* out) {
  if (M < 1 || M > 16 || N <= 0 || N % 16 || K <= 0 || K % kSkUnit || ncu <= 0) return 0;
  if (N / 16 > 0x7fffffffLL || K > 0x7fffffffLL) return 0;
  const int64_t tiles = N / 16, units = K / kSkUnit;
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

// the contract checks and the launch of both entry points; ldb in elements of W
template <typename Fmt>
int skinny_launch(const void* A, int64_t lda, const void* B, int64_t ldb, const void* wscale,
                  void* C, int64_t M, int64_t N, int64_t K, const void* bias,
                  const void* residual, int64_t ldr, int epi, int out_f32, int ncu,
                  hipStream_t stream) {
  int64_t plan[4];
  if (!skinny_plan(M, N, K, ncu, Fmt::kMinUnits, plan)) return hipErrorInvalidValue;
  constexpr int ldb_mult = 16 / static_cast<int>(sizeof(typename Fmt::Elem));   // 16 bytes
  if (!A || !B || !C || lda % 8 || ldb % ldb_mult || lda < K || ldb < K)
    return hipErrorInvalidValue;
  if (Fmt::kScaled && !wscale) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) |
       reinterpret_cast<uintptr_t>(C) | reinterpret_cast<uintptr_t>(wscale)) & 15)
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
               static_cast<int>((K / kSkUnit) / plan[1]), static_cast<int>((K / kSkUnit) % plan[1]),
               static_cast<const float*>(wscale)};
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
  return skinny_plan(M, N, K, ncu, WBf16::kMinUnits, out);
}

// The W8 form's plan: at least 4 units per wave. This kernel stays out of the autotuner.
DLBB_API int dlbb_gemm_w8_skinny_plan(int64_t M, int64_t N, int64_t K, int ncu, int64_t* out) {
  return skinny_plan(M, N, K, ncu, WE4m3::kMinUnits, out);
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
