// Global gradient-norm clipping over the trainer's flat gradient buffers, fused the way llm.c
// and nanoGPT's recipe need it (clip the global L2 norm, usually at 1.0) without a host sync and
// without a pass that rewrites the gradients:
//   1. grad_sumsq_kernel: one read-only HBM-streaming pass per reduced bucket, sum of g^2 into
//      ONE fp32 partial per workgroup (its slot). No atomics and no tickets: every reduction is a
//      fixed tree, so the partials are bit-identical from run to run.
//   2. clip_coef_kernel: one workgroup sums the partials of every bucket (fixed order) and leaves
//      norm, clip coefficient and the sum in device memory.
//   3. csrc/adam.hip's clip variants read the coefficient on the device.
// The whole chain replays as a HIP graph.
#include "common.h"

namespace dlbb {

constexpr int kSumsqBlock = 256;
// Slots (= most workgroups) per range and 16-byte loads in flight per lane, from the sweep in
// profiles/grad_clip/SUMMARY.md (tools/grad_clip_bench.py --sweep): every pair with >= 1 MiB in
// flight over the chip reads 64 MiB - 256 MiB at 6.0 - 7.2 TB/s (only 2 loads x 256 workgroups
// falls to 4.8 - 5.5); 8 loads x 512 workgroups was within 2 % of the best at each size, twice.
constexpr int kSumsqSlots = 512;
constexpr int kSumsqUnroll = 8;

// working workgroups for n elements: a function of n (and the unroll) alone, as stream_grid is
inline int sumsq_grid(int64_t n, int unroll, int cap) {
  const int64_t chunk = static_cast<int64_t>(kSumsqBlock) * unroll;    // 8-element vectors
  int64_t g = (n / 8 + chunk - 1) / chunk;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return static_cast<int>(g);
}

// workgroup sum in a fixed order: xor-butterfly inside the wave, then the waves' sums through
// LDS added in wave order by thread 0 (valid in thread 0 only)
__device__ __forceinline__ float block_sum_fixed(float v, float* lds) {
  v = wave_sum(v);
  const int wave = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == 0) lds[wave] = v;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0) {
    s = lds[0];
    for (int w = 1; w < kSumsqBlock / kWave; ++w) s += lds[w];
  }
  return s;
}

// Workgroup b sums the 8-element vectors [b*CH + k*grid*CH, +CH) for k = 0, 1, ... (CH = 256*U),
// U independent 16-byte loads per lane per step; lane accumulators are one per element position
// (8 chains of fma(x, x, acc): the square is not rounded). Workgroup 0 adds the n % 8 tail and
// zeroes the slots no workgroup owns.
template <int GDT, int U>
__global__ void __launch_bounds__(kSumsqBlock)
grad_sumsq_kernel(const void* __restrict__ g, int64_t n, float* __restrict__ partials,
                  int n_slots) {
  __shared__ float lds[kSumsqBlock / kWave];
  constexpr int64_t CH = static_cast<int64_t>(kSumsqBlock) * U;
  const int64_t nvec = n / 8;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * CH;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int64_t base = static_cast<int64_t>(blockIdx.x) * CH; base < nvec; base += stride) {
    float v[U][8];
    if (base + CH <= nvec) {            // wave-uniform: a full step keeps U loads in flight
#pragma unroll
      for (int u = 0; u < U; ++u) load8<GDT>(g, base + u * kSumsqBlock + threadIdx.x, v[u]);
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(v[u][j], v[u][j], acc[j]);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t i = base + u * kSumsqBlock + threadIdx.x;
        if (i < nvec) {
          load8<GDT>(g, i, v[u]);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(v[u][j], v[u][j], acc[j]);
        }
      }
    }
  }
  if (blockIdx.x == 0) {
    const int64_t t = nvec * 8 + threadIdx.x;
    if (threadIdx.x < 8 && t < n) {
      const float x = Elem<GDT>::ld(static_cast<const typename Elem<GDT>::T*>(g), t);
      acc[0] = __builtin_fmaf(x, x, acc[0]);
    }
    for (int s = gridDim.x + threadIdx.x; s < n_slots; s += kSumsqBlock) partials[s] = 0.f;
  }
  const float lane =
      ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  const float total = block_sum_fixed(lane, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// One workgroup: thread t sums partials t, t+256, ... in order, then the fixed workgroup tree.
// out[0] = norm = sqrt(sum) * pre_scale, out[1] = min(max_norm / (norm + 1e-6), 1), out[2] = sum
// (torch.nn.utils.clip_grad_norm_). A non-finite sum gives NaN norm and NaN coefficient, which
// the optimizer propagates (error_if_nonfinite=False). `out + 2` may alias `partials` (count 1).
__global__ void __launch_bounds__(kSumsqBlock)
clip_coef_kernel(const float* partials, int64_t count, float pre_scale, float max_norm,
                 float* out) {
  __shared__ float lds[kSumsqBlock / kWave];
  float v = 0.f;
  for (int64_t i = threadIdx.x; i < count; i += kSumsqBlock) v += partials[i];
  const float sum = block_sum_fixed(v, lds);
  if (threadIdx.x == 0) {
    float norm = sqrtf(sum) * pre_scale;
    float coef = max_norm / (norm + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;        // a NaN stays (fminf would return 1)
    if ((__float_as_uint(norm) & 0x7f800000u) == 0x7f800000u) {
      norm = __uint_as_float(0x7fc00000u);
      coef = norm;
    }
    out[0] = norm;
    out[1] = coef;
    out[2] = sum;
  }
}

template <int GDT>
static int launch_sumsq(const void* g, int64_t n, float* partials, int n_slots, int unroll,
                        int grid, hipStream_t stream) {
  const dim3 gr(grid), bl(kSumsqBlock);
  if (unroll == 2) {
    hipLaunchKernelGGL((grad_sumsq_kernel<GDT, 2>), gr, bl, 0, stream, g, n, partials, n_slots);
  } else if (unroll == 4) {
    hipLaunchKernelGGL((grad_sumsq_kernel<GDT, 4>), gr, bl, 0, stream, g, n, partials, n_slots);
  } else if (unroll == 8) {
    hipLaunchKernelGGL((grad_sumsq_kernel<GDT, 8>), gr, bl, 0, stream, g, n, partials, n_slots);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

static int sumsq_checked(const void* g, int dtype, int64_t n, float* partials, int n_slots,
                         int unroll, int grid_cap, hipStream_t stream) {
  if ((!g && n > 0) || !partials || n < 0 || n_slots < 1 || grid_cap < 1)
    return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(g) % 16 != 0) return hipErrorInvalidValue;
  if (unroll != 2 && unroll != 4 && unroll != 8) return hipErrorInvalidValue;
  const int grid = sumsq_grid(n, unroll, grid_cap);
  if (grid > n_slots) return hipErrorInvalidValue;     // every workgroup owns a slot
  if (dtype == DT_BF16) return launch_sumsq<DT_BF16>(g, n, partials, n_slots, unroll, grid, stream);
  if (dtype == DT_F32) return launch_sumsq<DT_F32>(g, n, partials, n_slots, unroll, grid, stream);
  return hipErrorInvalidValue;
}

}  // namespace dlbb

using namespace dlbb;

// Sum of squares of the contiguous bf16|fp32 range g[0, n) into partials[0, n_slots): slot b
// holds workgroup b's sum, the slots past the grid hold 0. `g` must be 16-byte aligned; n >= 0.
DLBB_API int dlbb_grad_sumsq(const void* g, int dtype, int64_t n, float* partials, int n_slots,
                             hipStream_t stream) {
  return sumsq_checked(g, dtype, n, partials, n_slots, kSumsqUnroll, kSumsqSlots, stream);
}

// The same pass with the loads in flight per lane (2, 4, 8) and the most workgroups chosen by
// the caller: the sweep behind the two defaults (tools/grad_clip_bench.py).
DLBB_API int dlbb_grad_sumsq_tune(const void* g, int dtype, int64_t n, float* partials,
                                  int n_slots, int unroll, int grid_cap, hipStream_t stream) {
  return sumsq_checked(g, dtype, n, partials, n_slots, unroll, grid_cap, stream);
}

// Launch geometry of dlbb_grad_sumsq for n elements: out4 = {workgroups, threads per workgroup,
// loads in flight per lane, slots per range}.
DLBB_API int dlbb_grad_sumsq_plan(int64_t n, int* out4) {
  if (!out4 || n < 0) return hipErrorInvalidValue;
  out4[0] = sumsq_grid(n, kSumsqUnroll, kSumsqSlots);
  out4[1] = kSumsqBlock;
  out4[2] = kSumsqUnroll;
  out4[3] = kSumsqSlots;
  return hipSuccess;
}

DLBB_API int dlbb_clip_coef(const float* partials, int64_t count, float pre_scale,
                            float max_norm, float* out, hipStream_t stream) {
  if (!partials || !out || count < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(kSumsqBlock), 0, stream, partials, count,
                     pre_scale, max_norm, out);
  return hipGetLastError();
}
