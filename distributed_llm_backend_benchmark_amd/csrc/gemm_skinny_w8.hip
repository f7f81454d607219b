// Skinny-M weight-only FP8 (W8A16) GEMM for the decode step's linears, gfx950.
//
//   out[M,N] = epilogue( (x[M,K] · Wq[N,K]^T) * wscale[n] ),  1 <= M <= 16, N % 16 == 0, K % 64 == 0
//   x bf16, Wq e4m3fn bytes (one fp32 scale per output row, ops.fp8.quantize_weight), fp32
//   accumulation; epilogue: (+ bias[N]) -> (GELU erf | GELU tanh) -> (+ residual[M,N]) ->
//   bf16 | fp32 store. The row scale multiplies the fp32 accumulator ahead of the bias, the order
//   of the FP8 GEMM (gemm_fp8.hip).
//
// The bf16 skinny kernel (gemm_skinny.hip) made a decode step a pure stream of W; this one
// streams half the bytes. Its structure is that kernel's: a workgroup owns 16 rows of W, its
// `kw` waves split K into contiguous ranges of 64-element units, W goes straight from global
// memory to VGPRs, the waves' 16 x 16 fp32 partial blocks are summed through LDS by wave 0 in
// wave order. No atomics, no workspace, no dependence on another workgroup: bit-identical from
// run to run and safe inside graph capture.
//
// The operand path differs:
//   * within a unit lane group q = l >> 4 reads the 16 contiguous bytes [16 q, 16 q + 16) of its W
//     row (one 16-B load) and the 16 bf16 [16 q, 16 q + 16) of its x row (two 16-B loads);
//   * the low and the high 8 bytes of the W load are widened to two bf16x8 operands with
//     v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 — one instruction per packed pair, 8 per unit (the
//     v_cvt_pk_f32_fp8 route needs 8 converts plus 8 v_perm_b32 to pack the high half-words).
//     e4m3fn has 3 mantissa bits and its exponent range lies inside bf16's, so the conversion is
//     exact (subnormals included);
//   * each operand feeds one v_mfma_f32_16x16x32_bf16 against the matching half of x: both
//     operands see the same k-permutation, which a dot product does not care about.
//
// Lanes whose x row is >= M read row 0 and store nothing (as the bf16 kernel): rows >= M of x are
// never read, rows >= M of out never written.
#include "common.h"

namespace dlbb {

namespace {

constexpr int W8_EPI_BIAS = 1, W8_EPI_GELU_ERF = 2, W8_EPI_GELU_TANH = 4, W8_EPI_RESIDUAL = 8;
constexpr int kW8Unit = 64;        // k elements per unit: two MFMAs, 16 B of W + 32 B of x per lane
constexpr int kW8MaxWaves = 16;    // waves per workgroup (1024 threads)
// units per batch of loads: 4 W + 8 x loads of 16 B per lane in flight ahead of the first wait
// (the bf16 kernel keeps 16), 48 VGPRs of operands, 72 in all. Measured against 2, 3, 5, 6 and 8
// units on the TP-7B shapes (docs/PERFORMANCE.md): 2 and 3 are no faster, 5 / 6 / 8 up to 14 / 6 /
// 23 % slower at world 1 — the wave ranges there are 4 or 16 units or 10-11, so deeper batches
// leave more to the tail batch, and their registers cost residency
constexpr int kW8Unroll = 4;
// A wave's K-range is at least this many units. A unit is 1 KiB of W per wave here, half the
// bf16 kernel's, so its minimum of 2 units would leave a wave 2 KiB to stream — half a batch of
// loads, all latency. 4 units keep the bf16 kernel's 4 KiB floor per wave and are one full batch
// (2 measured no faster on any row, 5 % slower at N = 4096, K = 512).
constexpr int kW8MinUnits = 4;
constexpr int kW8WavesPerCU = 16;  // the plan's target of resident waves per CU over the whole grid

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16v2 __attribute__((ext_vector_type(2)));

struct W8Args {
  const uint16_t* x;
  const uint8_t* w;
  const float* wscale;
  void* out;
  const uint16_t* bias;
  const uint16_t* residual;
  int64_t lda, ldw, ldr;
  int M, N, K;
  int epi;
  int out_f32;
  int kw;                          // waves per workgroup = K-split inside the workgroup
  int uq, ur;                      // units / kw, units % kw: wave w owns uq (+1 if w < ur) units
};

__device__ __forceinline__ bf16x8 ld16x(const uint16_t* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}
__device__ __forceinline__ u32x4 ld16w(const uint8_t* p) {
  return *reinterpret_cast<const u32x4*>(p);
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

__device__ __forceinline__ void unit_mfma(const u32x4& w, const bf16x8& x0, const bf16x8& x1,
                                          f32x4& acc0, f32x4& acc1) {
  acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(widen8(w[0], w[1]), x0, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(widen8(w[2], w[3]), x1, acc1, 0, 0, 0);
}

__global__ __launch_bounds__(kW8MaxWaves * 64) void gemm_w8_nt_skinny_kernel(W8Args a) {
  extern __shared__ f32x4 w8_part[];            // [kw][64 lanes] partial blocks
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * 16;
  // wave's contiguous unit range (balanced; every wave has >= kW8MinUnits by the plan)
  const int u0 = wave * a.uq + (wave < a.ur ? wave : a.ur);
  const int u1 = u0 + a.uq + (wave < a.ur ? 1 : 0);
  const int xr = fr < a.M ? fr : 0;
  const uint8_t* wp = a.w + static_cast<int64_t>(n0 + fr) * a.ldw + fq * 16;
  const uint16_t* xp = a.x + static_cast<int64_t>(xr) * a.lda + fq * 16;

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int u = u0;
  for (; u + kW8Unroll <= u1; u += kW8Unroll) {
    u32x4 wf[kW8Unroll];
    bf16x8 xf[kW8Unroll][2];
#pragma unroll
    for (int i = 0; i < kW8Unroll; ++i) wf[i] = ld16w(wp + (u + i) * kW8Unit);
#pragma unroll
    for (int i = 0; i < kW8Unroll; ++i) {
      xf[i][0] = ld16x(xp + (u + i) * kW8Unit);
      xf[i][1] = ld16x(xp + (u + i) * kW8Unit + 8);
    }
    __builtin_amdgcn_sched_barrier(0);          // the whole batch is in flight before any wait
#pragma unroll
    for (int i = 0; i < kW8Unroll; ++i) unit_mfma(wf[i], xf[i][0], xf[i][1], acc0, acc1);
  }
  if (u < u1) {
    // the last 1 .. kW8Unroll - 1 units as one batch too: a slot past the range loads the
    // range's last unit again (in bounds, the same addresses) and its MFMAs are skipped
    const int rem = u1 - u;                     // wave-uniform
    u32x4 wf[kW8Unroll - 1];
    bf16x8 xf[kW8Unroll - 1][2];
#pragma unroll
    for (int i = 0; i < kW8Unroll - 1; ++i) {
      const int ui = u + (i < rem ? i : rem - 1);
      wf[i] = ld16w(wp + ui * kW8Unit);
      xf[i][0] = ld16x(xp + ui * kW8Unit);
      xf[i][1] = ld16x(xp + ui * kW8Unit + 8);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kW8Unroll - 1; ++i) {
      if (i < rem) unit_mfma(wf[i], xf[i][0], xf[i][1], acc0, acc1);
    }
  }
  f32x4 v = acc0 + acc1;

  if (a.kw > 1) {                               // wave-uniform
    w8_part[wave * 64 + lane] = v;
    __syncthreads();
    if (wave != 0) return;
    v = w8_part[lane];
    for (int s = 1; s < a.kw; ++s) v += w8_part[s * 64 + lane];   // fixed order
  }
  if (fr >= a.M) return;                        // padding columns of the MFMA: nothing stored

  const int n = n0 + fq * 4;
  const int epi = a.epi;
  v *= *reinterpret_cast<const f32x4*>(a.wscale + n);
  if (epi & W8_EPI_BIAS) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += bf16_to_f32(a.bias[n + r]);
  }
  if (epi & W8_EPI_GELU_ERF) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = gelu_erf(v[r]);
  } else if (epi & W8_EPI_GELU_TANH) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = gelu_tanh(v[r]);
  }
  if (epi & W8_EPI_RESIDUAL) {
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

}  // namespace

}  // namespace dlbb

using namespace dlbb;

// Plan of the W8 skinny GEMM, the meaning of dlbb_gemm_skinny_plan: out = {grid (workgroups, one
// per 16 rows of Wq), K-split inside a workgroup (waves), K-split across workgroups (always 1),
// workspace bytes (always 0)}; returns 0 outside the contract. ~16 waves per CU over the whole
// grid with at least kW8MinUnits units per wave.
DLBB_API int dlbb_gemm_w8_skinny_plan(int64_t M, int64_t N, int64_t K, int ncu, int64_t* out) {
  if (M < 1 || M > 16 || N <= 0 || N % 16 || K <= 0 || K % kW8Unit || ncu <= 0) return 0;
  if (N / 16 > 0x7fffffffLL || K > 0x7fffffffLL) return 0;
  const int64_t tiles = N / 16, units = K / kW8Unit;
  int64_t kw = (static_cast<int64_t>(ncu) * kW8WavesPerCU + tiles - 1) / tiles;
  if (kw > units / kW8MinUnits) kw = units / kW8MinUnits;
  if (kw > kW8MaxWaves) kw = kW8MaxWaves;
  if (kw < 1) kw = 1;
  out[0] = tiles;
  out[1] = kw;
  out[2] = 1;
  out[3] = 0;
  return 1;
}

// out[M, N] = act((A[M, K] · Bq[N, K]^T) * wscale[N] + bias) + residual on the caller's stream;
// A bf16, Bq e4m3fn bytes, wscale fp32, `out` contiguous (row stride N), bf16 or fp32 (out_f32).
// Outside the contract (1 <= M <= 16, N % 16 == 0, K % 64 == 0, lda a multiple of 8 elements,
// ldb a multiple of 16 bytes, both >= K, 16-byte aligned A / Bq / out / wscale, epi within
// bias | GELU | residual with at most one GELU, non-null pointers for what epi names) nothing is
// launched and hipErrorInvalidValue is returned.
DLBB_API int dlbb_gemm_w8_nt_skinny(const void* A, int64_t lda, const void* Bq, int64_t ldb,
                                    const void* wscale, void* C, int64_t M, int64_t N, int64_t K,
                                    const void* bias, const void* residual, int64_t ldr, int epi,
                                    int out_f32, int ncu, hipStream_t stream) {
  int64_t plan[4];
  if (!dlbb_gemm_w8_skinny_plan(M, N, K, ncu, plan)) return hipErrorInvalidValue;
  if (!A || !Bq || !C || !wscale || lda % 8 || ldb % 16 || lda < K || ldb < K)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Bq) |
       reinterpret_cast<uintptr_t>(C) | reinterpret_cast<uintptr_t>(wscale)) & 15)
    return hipErrorInvalidValue;
  if (epi & ~(W8_EPI_BIAS | W8_EPI_GELU_ERF | W8_EPI_GELU_TANH | W8_EPI_RESIDUAL))
    return hipErrorInvalidValue;
  if ((epi & W8_EPI_GELU_ERF) && (epi & W8_EPI_GELU_TANH)) return hipErrorInvalidValue;
  if ((epi & W8_EPI_BIAS) && !bias) return hipErrorInvalidValue;
  if ((epi & W8_EPI_RESIDUAL) && (!residual || ldr < N)) return hipErrorInvalidValue;
  W8Args a{static_cast<const uint16_t*>(A), static_cast<const uint8_t*>(Bq),
           static_cast<const float*>(wscale), C, static_cast<const uint16_t*>(bias),
           static_cast<const uint16_t*>(residual), lda, ldb, ldr, static_cast<int>(M),
           static_cast<int>(N), static_cast<int>(K), epi, out_f32, static_cast<int>(plan[1]),
           static_cast<int>((K / kW8Unit) / plan[1]), static_cast<int>((K / kW8Unit) % plan[1])};
  const dim3 g(static_cast<unsigned>(plan[0])), b(static_cast<unsigned>(plan[1] * 64));
  const size_t lds = plan[1] > 1 ? static_cast<size_t>(plan[1]) * 64 * sizeof(f32x4) : 0;
  hipLaunchKernelGGL(gemm_w8_nt_skinny_kernel, g, b, lds, stream, a);
  return hipGetLastError();
}
