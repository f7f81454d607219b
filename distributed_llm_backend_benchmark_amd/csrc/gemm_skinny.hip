// Skinny-M weight-streaming bf16 GEMM for the decode step's linears, gfx950.
//
//   out[M,N] = epilogue( x[M,K] · W[N,K]^T ),  1 <= M <= 16, N % 16 == 0, K % 64 == 0
//   epilogue: (+ bias[N]) -> (GELU erf | GELU tanh) -> (+ residual[M,N]) -> bf16 | fp32 store
//   (the meaning of dlbb_gemm_bf16_nt_v without the pre-activation output, which is training
//   only).
//
// At M = batch rows the 256² / 128² tiles of gemm.hip are > 90 % padding and the step is a pure
// stream of W. This kernel reads W exactly once, straight from global memory into VGPRs (16 B
// per lane, a batch of 16 loads in flight, then counted waits) — no LDS staging: nothing is shared between
// waves, so the LDS round trip would be pure overhead.
//
//   * A workgroup owns 16 rows of W (one column tile of out); its `kw` waves split K into
//     contiguous ranges of 64-element units.
//   * v_mfma_f32_16x16x32_bf16 with A = W (row = lane & 15) and B = x^T (column = lane & 15 = the
//     row m of x), so lane l ends with out[m = l & 15][n0 + 4 (l >> 4) + 0..3]: four contiguous
//     outputs per lane, one 16-byte (fp32) or 8-byte (bf16) store.
//   * The dot product does not care about the order of k: within a unit lane group q = l >> 4
//     reads the 32 contiguous bytes [32 q, 32 q + 32) of its W row (two 16-B loads) and the
//     same bytes of its x row, so both MFMAs of the unit see one k-permutation on both operands.
//   * Lanes whose x row is >= M read row 0 instead (always valid; the same addresses as the
//     lanes of row 0, so no extra traffic). Their MFMA columns hold garbage that no other
//     column depends on, and they store nothing: rows >= M of x are never read, rows >= M of
//     out never written.
//   * The waves' 16 x 16 fp32 partial blocks are summed through LDS by wave 0 in wave order — a
//     fixed order, so results are bit-identical from run to run. No atomics, no device
//     workspace, no dependence on any other workgroup: safe beside communication kernels and
//     inside graph capture.
#include "common.h"

namespace dlbb {

namespace {

constexpr int SK_EPI_BIAS = 1, SK_EPI_GELU_ERF = 2, SK_EPI_GELU_TANH = 4, SK_EPI_RESIDUAL = 8;
constexpr int kSkUnit = 64;        // k elements per unit: two MFMAs, 32 B per lane per operand
constexpr int kSkMaxWaves = 16;    // waves per workgroup (1024 threads)
constexpr int kSkUnroll = 4;       // units per batch of loads: 8 W + 8 x loads of 16 B in flight
constexpr int kSkMinUnits = 2;     // a wave's K-range is at least this many units

struct SkinnyArgs {
  const uint16_t* x;
  const uint16_t* w;
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

__device__ __forceinline__ bf16x8 ld16(const uint16_t* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}

__global__ __launch_bounds__(kSkMaxWaves * 64) void gemm_bf16_nt_skinny_kernel(SkinnyArgs a) {
  extern __shared__ f32x4 sk_part[];            // [kw][64 lanes] partial blocks
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * 16;
  // wave's contiguous unit range (balanced; every wave has >= kSkMinUnits by the plan)
  const int u0 = wave * a.uq + (wave < a.ur ? wave : a.ur);
  const int u1 = u0 + a.uq + (wave < a.ur ? 1 : 0);
  const int xr = fr < a.M ? fr : 0;
  const uint16_t* wp = a.w + static_cast<int64_t>(n0 + fr) * a.ldw + fq * 16;
  const uint16_t* xp = a.x + static_cast<int64_t>(xr) * a.lda + fq * 16;

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  int u = u0;
  for (; u + kSkUnroll <= u1; u += kSkUnroll) {
    bf16x8 wf[kSkUnroll][2], xf[kSkUnroll][2];
#pragma unroll
    for (int i = 0; i < kSkUnroll; ++i) {
      wf[i][0] = ld16(wp + (u + i) * kSkUnit);
      wf[i][1] = ld16(wp + (u + i) * kSkUnit + 8);
    }
#pragma unroll
    for (int i = 0; i < kSkUnroll; ++i) {
      xf[i][0] = ld16(xp + (u + i) * kSkUnit);
      xf[i][1] = ld16(xp + (u + i) * kSkUnit + 8);
    }
    __builtin_amdgcn_sched_barrier(0);          // the whole batch is in flight before any wait
#pragma unroll
    for (int i = 0; i < kSkUnroll; ++i) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i][0], xf[i][0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i][1], xf[i][1], acc1, 0, 0, 0);
    }
  }
  for (; u < u1; ++u) {
    const bf16x8 w0 = ld16(wp + u * kSkUnit), w1 = ld16(wp + u * kSkUnit + 8);
    const bf16x8 x0 = ld16(xp + u * kSkUnit), x1 = ld16(xp + u * kSkUnit + 8);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w0, x0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1, x1, acc1, 0, 0, 0);
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

}  // namespace

}  // namespace dlbb

using namespace dlbb;

// Plan of the skinny GEMM for an [M, K] x [N, K]^T shape on `ncu` CUs: out = {grid (workgroups,
// one per 16 rows of W), K-split inside a workgroup (waves), K-split across workgroups (always
// 1: this kernel has no cross-workgroup combine), workspace bytes (always 0)}; returns 0 outside
// the contract. The in-workgroup split aims at ~16 waves per CU over the whole grid with at
// least kSkMinUnits 64-element units per wave.
DLBB_API int dlbb_gemm_skinny_plan(int64_t M, int64_t N, int64_t K, int ncu, int64_t* out) {
  if (M < 1 || M > 16 || N <= 0 || N % 16 || K <= 0 || K % kSkUnit || ncu <= 0) return 0;
  if (N / 16 > 0x7fffffffLL || K > 0x7fffffffLL) return 0;
  const int64_t tiles = N / 16, units = K / kSkUnit;
  int64_t kw = (static_cast<int64_t>(ncu) * 16 + tiles - 1) / tiles;
  if (kw > units / kSkMinUnits) kw = units / kSkMinUnits;
  if (kw > kSkMaxWaves) kw = kSkMaxWaves;
  if (kw < 1) kw = 1;
  out[0] = tiles;
  out[1] = kw;
  out[2] = 1;
  out[3] = 0;
  return 1;
}

// out[M, N] = act(A[M, K] · B[N, K]^T + bias) + residual on the caller's stream; `out` is
// contiguous (row stride N), bf16 or fp32 (out_f32). Outside the contract (1 <= M <= 16,
// N % 16 == 0, K % 64 == 0, lda / ldb multiples of 8 elements, 16-byte aligned A / B / out, epi
// within bias | GELU | residual) nothing is launched and hipErrorInvalidValue is returned.
DLBB_API int dlbb_gemm_bf16_nt_skinny(const void* A, int64_t lda, const void* B, int64_t ldb,
                                      void* C, int64_t M, int64_t N, int64_t K, const void* bias,
                                      const void* residual, int64_t ldr, int epi, int out_f32,
                                      int ncu, hipStream_t stream) {
  int64_t plan[4];
  if (!dlbb_gemm_skinny_plan(M, N, K, ncu, plan)) return hipErrorInvalidValue;
  if (!A || !B || !C || lda % 8 || ldb % 8 || lda < K || ldb < K) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) |
       reinterpret_cast<uintptr_t>(C)) & 15)
    return hipErrorInvalidValue;
  if (epi & ~(SK_EPI_BIAS | SK_EPI_GELU_ERF | SK_EPI_GELU_TANH | SK_EPI_RESIDUAL))
    return hipErrorInvalidValue;
  if ((epi & SK_EPI_GELU_ERF) && (epi & SK_EPI_GELU_TANH)) return hipErrorInvalidValue;
  if ((epi & SK_EPI_BIAS) && !bias) return hipErrorInvalidValue;
  if ((epi & SK_EPI_RESIDUAL) && (!residual || ldr < N)) return hipErrorInvalidValue;
  SkinnyArgs a{static_cast<const uint16_t*>(A), static_cast<const uint16_t*>(B), C,
               static_cast<const uint16_t*>(bias), static_cast<const uint16_t*>(residual),
               lda, ldb, ldr, static_cast<int>(M), static_cast<int>(N), static_cast<int>(K),
               epi, out_f32, static_cast<int>(plan[1]),
               static_cast<int>((K / kSkUnit) / plan[1]), static_cast<int>((K / kSkUnit) % plan[1])};
  const dim3 g(static_cast<unsigned>(plan[0])), b(static_cast<unsigned>(plan[1] * 64));
  const size_t lds = plan[1] > 1 ? static_cast<size_t>(plan[1]) * 64 * sizeof(f32x4) : 0;
  hipLaunchKernelGGL(gemm_bf16_nt_skinny_kernel, g, b, lds, stream, a);
  return hipGetLastError();
}
