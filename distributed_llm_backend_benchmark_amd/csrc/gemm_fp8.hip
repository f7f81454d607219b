// FP8 (OCP e4m3fn) path of the tensor-parallel forward, gfx950: a one-pass row quantiser and an
// NT GEMM on the block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4, twice the bf16 MFMA rate).
//
//   quantiser: q[m, :] = e4m3fn_rne(float(x[m, :]) * (448 / amax_m)), scale[m] = amax_m / 448
//   GEMM:      C[M,N] = epilogue( (A8[M,K] · B8[N,K]^T) * sa[m] * sb[n] )
//              epilogue: (+ bias[N]) -> (GELU erf | GELU tanh) -> (+ residual[M,N]) -> bf16 | fp32
//
// The GEMM is the 256 x 256 ping-pong schedule of csrc/gemm.hip (pingpong_body, NT) with the
// K-tile redefined as 128 e4m3 elements: a 256 x 128 e4m3 tile has 128-byte rows exactly like
// the 256 x 64 bf16 tile, so the LDS-DMA staging (buffer_load ... lds, 16 B per lane), the
// 16-byte-slot XOR swizzle, the 160 KiB A-double / B-triple buffer plan and every counted vmcnt
// wait carry over byte for byte; the helpers are copied here (gemm.hip is left untouched). What
// changes is the fragment (32 B per lane: two swizzled 16-B slots) and the MFMA: 32 per wave
// and K-tile instead of 64, each over K = 128.
// The per-row dequantisation scales are applied in the epilogue; the hardware block scales are
// all 1.0 (E8M0 byte 127).
#include "common.h"

namespace dlbb {
namespace fp8 {

typedef int i32x8 __attribute__((ext_vector_type(8)));     // scaled-MFMA operand: 32 e4m3 bytes
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

enum Epi : int { EPI_BIAS = 1, EPI_GELU_ERF = 2, EPI_GELU_TANH = 4, EPI_RESIDUAL = 8 };

// ---------------------------------------------------------------------------------------
// Row quantiser. A row is read from memory ONCE: every thread keeps its NV 16-byte vectors
// (8 bf16 each) in registers between the amax reduction and the convert.
//   WAVE_ROW: one wave per row (4 rows per 256-thread workgroup), K <= 64 * 8 * NV
//   else:     one workgroup per row,                              K <= 256 * 8 * NV
// amax == 0: scale 1, bytes 0. Otherwise inv = 448 / amax and scale = amax / 448 are IEEE fp32
// divisions (hipcc's default correctly rounded `/`), q = cvt_pk_fp8_f32(x * inv): one fp32
// multiply, round to nearest even. Non-finite inputs are outside the contract.
constexpr int kQThreads = 256;

template <bool WAVE_ROW, int NV>
__global__ void __launch_bounds__(kQThreads) quant_fp8_rows_kernel(
    const uint16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ q, int64_t ldq,
    float* __restrict__ scale, int64_t M, int K8) {
  __shared__ float part[kQThreads / kWave];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = WAVE_ROW ? static_cast<int64_t>(blockIdx.x) * (kQThreads / kWave) + wave
                               : static_cast<int64_t>(blockIdx.x);
  const int t = WAVE_ROW ? lane : static_cast<int>(threadIdx.x);
  constexpr int kStride = WAVE_ROW ? kWave : kQThreads;
  const bool live = row < M;                       // wave-uniform
  const u16x8* xr = reinterpret_cast<const u16x8*>(x + (live ? row : 0) * ldx);
  u16x8 v[NV];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = t + i * kStride;
    v[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (live && c < K8) v[i] = xr[c];
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = __builtin_fmaxf(amax, __builtin_fabsf(bf16_to_f32(v[i][j])));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax = __builtin_fmaxf(amax, __shfl_xor(amax, o, 64));
  if constexpr (!WAVE_ROW) {
    if (lane == 0) part[wave] = amax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kQThreads / kWave; ++w) amax = __builtin_fmaxf(amax, part[w]);
  }
  if (!live) return;
  const bool zero = amax == 0.f;
  const float inv = zero ? 1.0f : 448.0f / amax;
  if (t == 0) scale[row] = zero ? 1.0f : amax / 448.0f;
  i32x2* qr = reinterpret_cast<i32x2*>(q + row * ldq);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = t + i * kStride;
    if (c >= K8) continue;
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = bf16_to_f32(v[i][j]) * inv;
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
    qr[c] = i32x2{lo, hi};
  }
}

// ---------------------------------------------------------------------------------------
// GEMM. Tile geometry in BYTES (identical to the bf16 ping-pong: 128-byte rows).
constexpr int BM2 = 256, BN2 = 256;
constexpr int BK8 = 128;                       // K-tile in e4m3 elements = row bytes
constexpr int kThreads2 = 512;
constexpr int kTile2Bytes = BM2 * BK8;         // 32 KiB per operand
constexpr int kPP6Lds = 5 * kTile2Bytes;       // A double + B triple = 160 KiB
constexpr int kGroupM = 8;

struct Fp8Args {
  const uint8_t* A;        // [M, K] e4m3, row stride lda bytes
  const uint8_t* B;        // [N, K] e4m3, row stride ldb bytes
  void* C;                 // [M, N] bf16 | fp32, row stride ldc elements
  const float* sa;         // [M]
  const float* sb;         // [N]
  const uint16_t* bias;    // [N] bf16
  const uint16_t* residual;  // [M, N] bf16, row stride ldr
  int64_t M, N, K;
  int64_t lda, ldb, ldc, ldr;
  int epi;
  int out_f32;
};

struct Tile256 {
  int64_t m0, n0;
};

// virtual workgroup id -> output tile: XCD-aware bijective remap, then GROUP_M ordering
__device__ __forceinline__ Tile256 tile_of(const Fp8Args& a, int vb) {
  const int tiles_m = static_cast<int>((a.M + BM2 - 1) / BM2);
  const int tiles_n = static_cast<int>((a.N + BN2 - 1) / BN2);
  const int nwg = tiles_m * tiles_n;
  const int q = nwg >> 3, r = nwg & 7, x = vb & 7;
  const int wid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (vb >> 3);
  const int group_size = kGroupM * tiles_n;
  const int group = wid / group_size;
  const int first_m = group * kGroupM;
  const int gm = (tiles_m - first_m) < kGroupM ? (tiles_m - first_m) : kGroupM;
  const int in_group = wid - group * group_size;
  return Tile256{static_cast<int64_t>(first_m + in_group % gm) * BM2,
                 static_cast<int64_t>(in_group / gm) * BN2};
}

__device__ __forceinline__ void bldsx4(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff,
                                       char* lds_base_wave_uniform) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)(lds_base_wave_uniform), 16, voff, soff,
                                           0, 0);
}

// B rows are staged PERMUTED inside each 64-row block (LDS row j*16 + t holds output column
// (t>>2)*16 + j*4 + (t&3)), so with the MFMA operands swapped every lane ends with 16
// consecutive output columns of one row (see store_tile)
__device__ __forceinline__ int perm_brow(int x) {
  return (x & ~63) | (((x >> 2) & 3) << 4) | (((x >> 4) & 3) << 2) | (x & 3);
}

// half (128 rows) of an A tile: 4 wave-instructions (8 rows x 128 B) per wave of the wave row.
// Ragged M (M % 8 == 0): 8-row groups past the end re-read the last group (stores are masked).
__device__ __forceinline__ void stage_a_half(__amdgpu_buffer_rsrc_t ra, uint32_t lda, int rows_a,
                                             uint32_t k0, char* abuf, int half, int w4,
                                             uint32_t aoff) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int trow = half * 128 + (i * 4 + w4) * 8;
    const int g = trow < rows_a - 8 ? trow : rows_a - 8;
    bldsx4(ra, aoff, static_cast<uint32_t>(g) * lda + k0, abuf + trow * BK8);
  }
}

// slice [I0, I1) of the 8 wave-instructions of a B tile (0..3 = tile rows [0, 128), 4..7 =
// [128, 256)). Ragged N (N % 64 == 0): 64-row blocks past the end re-read block 0.
template <int I0, int I1>
__device__ __forceinline__ void stage_b(__amdgpu_buffer_rsrc_t rb, uint32_t ldb, int rows_b,
                                        uint32_t k0, char* bbuf, int w4, uint32_t boff) {
#pragma unroll
  for (int i = I0; i < I1; ++i) {
    const int trow = (i * 4 + w4) * 8;
    const int g = (trow & ~63) < rows_b ? perm_brow(trow) : (perm_brow(trow) & 63);
    bldsx4(rb, boff, static_cast<uint32_t>(g) * ldb + k0, bbuf + trow * BK8);
  }
}

// One lane's operand of v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3): 32 bytes of tile row `row`.
// Operand lane map, established on the GPU with exact small-integer data (asymmetric B, an A
// pattern that differs per row and per k; tests/test_fp8_gemm_gpu.py): lane l supplies matrix row
// l & 15 and 32 of the instruction's 128 k, and byte b of A-lane (row i, group g = l >> 4) is
// multiplied with byte b of B-lane (row j, group g) — A and B cut K the same way, so the product
// is right for ANY 32-byte slice of the K-tile per lane group as long as both operands take the
// same one. Group g takes the contiguous k [32 g, 32 g + 32): in LDS the two swizzled 16-byte
// slots (2 g) ^ (row & 7) and that ^ 1. With the operands swapped (B tile first) the C/D map is
// the 16x16 one of every dtype: register r of lane l = B-tile row 4 (l >> 4) + r, A-tile row l & 15.
__device__ __forceinline__ i32x8 read_frag(const char* lds, int row, int fq) {
  const int off = row * BK8 + (((2 * fq) ^ (row & 7)) << 4);
  const i32x4 lo = *reinterpret_cast<const i32x4*>(lds + off);
  const i32x4 hi = *reinterpret_cast<const i32x4*>(lds + (off ^ 16));
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N <= 63, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ float apply_act(float v, int epi) {
  if (epi & EPI_GELU_ERF) return gelu_erf(v);
  if (epi & EPI_GELU_TANH) return gelu_tanh(v);
  return v;
}

// Epilogue of one wave's 128 x 64 block at (row0, col0): lane (fr, fq) holds output rows
// row0 + 16 i + fr, columns col0 + 16 fq + 4 j + r in acc[i][j][r]. All rows are 16-byte aligned
// and N % 64 == 0 (host contract), so every access is a whole 16-byte vector.
__device__ __forceinline__ void store_tile(const Fp8Args& a, const f32x4 (&acc)[8][4],
                                           int64_t row0, int64_t col0, int lane) {
  const int fr = lane & 15, fq = lane >> 4;
  const int epi = a.epi;
  const int64_t cbase = col0 + fq * 16;
  if (cbase >= a.N) return;
  const int64_t rbase = row0 + fr;
  const int rows_left = static_cast<int>(a.M - rbase);
  float sb[16], bias[16];
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const f32x4 s = reinterpret_cast<const f32x4*>(a.sb + cbase)[qd];
#pragma unroll
    for (int c = 0; c < 4; ++c) sb[4 * qd + c] = s[c];
  }
#pragma unroll
  for (int c = 0; c < 16; ++c) bias[c] = 0.f;
  if (epi & EPI_BIAS) {
    const u16x8* bp = reinterpret_cast<const u16x8*>(a.bias + cbase);
    const u16x8 b0v = bp[0], b1v = bp[1];
#pragma unroll
    for (int c = 0; c < 8; ++c) { bias[c] = bf16_to_f32(b0v[c]); bias[8 + c] = bf16_to_f32(b1v[c]); }
  }
  float* cf = static_cast<float*>(a.C) + rbase * a.ldc + cbase;
  uint16_t* cb = static_cast<uint16_t*>(a.C) + rbase * a.ldc + cbase;
  const uint16_t* rb = (epi & EPI_RESIDUAL) ? a.residual + rbase * a.ldr + cbase : nullptr;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i * 16 >= rows_left) break;
    const float sa = a.sa[rbase + i * 16];
    float v[16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        v[j * 4 + r] = (acc[i][j][r] * sa) * sb[j * 4 + r] + bias[j * 4 + r];
    const int64_t oc = static_cast<int64_t>(i) * 16 * a.ldc, orr = static_cast<int64_t>(i) * 16 * a.ldr;
    if (epi & (EPI_GELU_ERF | EPI_GELU_TANH)) {
#pragma unroll
      for (int c = 0; c < 16; ++c) v[c] = apply_act(v[c], epi);
    }
    if (rb) {
      const u16x8 r0 = reinterpret_cast<const u16x8*>(rb + orr)[0];
      const u16x8 r1 = reinterpret_cast<const u16x8*>(rb + orr)[1];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        v[c] += bf16_to_f32(r0[c]);
        v[8 + c] += bf16_to_f32(r1[c]);
      }
    }
    if (a.out_f32) {
      float4* o = reinterpret_cast<float4*>(cf + oc);
#pragma unroll
      for (int qd = 0; qd < 4; ++qd)
        o[qd] = make_float4(v[4 * qd], v[4 * qd + 1], v[4 * qd + 2], v[4 * qd + 3]);
    } else {
      u16x8 o0, o1;
#pragma unroll
      for (int c = 0; c < 8; ++c) { o0[c] = f32_to_bf16(v[c]); o1[c] = f32_to_bf16(v[8 + c]); }
      reinterpret_cast<u16x8*>(cb + oc)[0] = o0;
      reinterpret_cast<u16x8*>(cb + oc)[1] = o1;
    }
  }
}

// The ping-pong schedule (csrc/gemm.hip pingpong_body, NT): 8 waves as 2 wave rows x 4 wave
// columns, 128 x 64 outputs per wave; the wave rows alternate between a memory interval (fragment
// reads + LDS-DMA issue) and an MFMA interval. A rows [0, 128) are read only by wave row 0 and
// rows [128, 256) only by wave row 1, so each A buffer is refilled in halves:
//   interval 2u   (row 0 reads tile u):  row 0 issues A-hi(u+1) and B(u+2)
//   interval 2u+1 (row 1 reads tile u):  row 1 issues A-lo(u+2)
// Waits are counted (oldest first) and the barriers raw, so the LDS-DMA stays in flight across
// them: row 0 ends interval 2u with A-hi(u) retired and 2u+1 with B(u+1) retired; row 1 ends
// 2u+1 with A-lo(u+1) retired. WAR: A-hi(u+1) replaces A-hi(u-1), B(u+2) replaces B(u-1) (both
// last read in interval 2u-1), A-lo(u+2) replaces A-lo(u) (row 0, 2u) — each behind the barrier
// that closes the read.
// BAL: the second half of every B tile from tile 2 on is issued by wave row 1 next to A-lo(u+2),
// so both rows issue 8 DMA instructions per K-tile; row 1 retires A-lo(u+1) and B1(u+1) together.
template <bool BAL>
__device__ __forceinline__ void pingpong_body(const Fp8Args& a, char* smem) {
  constexpr int NBI = 8;                      // B DMA instructions per staging wave per K-tile
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int fr = lane & 15, fq = lane >> 4;
  const Tile256 tl = tile_of(a, static_cast<int>(blockIdx.x));
  const int64_t m0 = tl.m0, n0 = tl.n0;
  const int nk = static_cast<int>(a.K / BK8);
  char* const abuf0 = smem;
  char* const bbuf0 = smem + 2 * kTile2Bytes;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  i32x8 af[8], bf[4];
  // LDS slot s of row r holds the 16-byte k-chunk s ^ (r & 7): swizzle on the SOURCE address
  const int r_in = lane >> 3, chunk = (lane & 7) ^ (lane >> 3);
  const uint32_t lda = static_cast<uint32_t>(a.lda), ldb = static_cast<uint32_t>(a.ldb);
  const uint32_t aoff = static_cast<uint32_t>(r_in) * lda + chunk * 16;
  const uint32_t boff = static_cast<uint32_t>(perm_brow(r_in)) * ldb + chunk * 16;
  const int rows_a = static_cast<int>(a.M - m0), rows_b = static_cast<int>(a.N - n0);
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(a.A + m0 * a.lda), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(a.B + n0 * a.ldb), 0, 0x7fffffff, 0x00020000);
  constexpr uint32_t kStep = BK8;

  auto read_frags = [&](const char* ab, const char* bb, int row) {
#pragma unroll
    for (int i = 0; i < 8; ++i) af[i] = read_frag(ab, row * 128 + i * 16 + fr, fq);
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = read_frag(bb, wc * 64 + j * 16 + fr, fq);
  };
  // operands swapped (D = W rows x X rows^T): a lane's 4 accumulator registers are 4 consecutive
  // output columns. Format codes 0 = e4m3 for both operands; scale byte 127 = 2^0 for both.
  auto mfma_all = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bf[j], af[i], acc[i][j], 0, 0,
                                                                     0, 127, 0, 127);
    // the MFMAs touch no memory, so nothing else keeps the compiler from sinking them below the
    // counted waits and the barrier that close their interval (it did): tie every accumulator
    // to an empty volatile asm, which stays in order with the wait / barrier asm statements
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) tr_tie(acc[i][j]);
  };

  if (wr == 0) {
    // prologue, row 0: A-lo(0), B(0), B(1); retire the first two
    stage_a_half(ra, lda, rows_a, 0, abuf0, 0, wc, aoff);
    stage_b<0, NBI>(rb, ldb, rows_b, 0, bbuf0, wc, boff);
    if (nk > 1) {
      stage_b<0, NBI>(rb, ldb, rows_b, kStep, bbuf0 + kTile2Bytes, wc, boff);
      wait_vm<NBI>();
    } else {
      wait_vm<0>();
    }
    __builtin_amdgcn_s_barrier();
    int cb = 0;                                       // B buffer of tile u
    for (int u = 0; u < nk; ++u) {
      const char* ab = abuf0 + (u & 1) * kTile2Bytes;
      read_frags(ab, bbuf0 + cb * kTile2Bytes, 0);
      const bool h1 = u + 1 < nk, b2 = u + 2 < nk;
      if (h1)
        stage_a_half(ra, lda, rows_a, (u + 1) * kStep, abuf0 + ((u + 1) & 1) * kTile2Bytes, 1, wc,
                     aoff);
      if (b2) {
        const int cb2 = cb == 0 ? 2 : cb - 1;         // (u + 2) % 3
        if (BAL)
          stage_b<0, NBI / 2>(rb, ldb, rows_b, (u + 2) * kStep, bbuf0 + cb2 * kTile2Bytes, wc, boff);
        else
          stage_b<0, NBI>(rb, ldb, rows_b, (u + 2) * kStep, bbuf0 + cb2 * kTile2Bytes, wc, boff);
      }
      // retire A-hi(u) (issued two intervals ago; tile 0's came from row 1)
      constexpr int kB2 = BAL ? NBI / 2 : NBI;        // B(u+2) instructions issued
      if constexpr (BAL) {
        if (b2) wait_vm<NBI / 2 + 4 + kB2>();
        else if (h1) wait_vm<NBI / 2 + 4>();
        else wait_vm<0>();
      } else {
        if (b2) wait_vm<NBI + 4 + kB2>();
        else if (h1) wait_vm<NBI + 4>();
        else wait_vm<0>();
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();                   // end of interval 2u
      __builtin_amdgcn_sched_barrier(0);
      mfma_all();
      __builtin_amdgcn_sched_barrier(0);
      if (h1) {                                       // retire B(u+1) (BAL: its first half)
        if (b2) { if (BAL) wait_vm<4 + NBI / 2>(); else wait_vm<4 + NBI>(); }
        else wait_vm<4>();
      }
      __builtin_amdgcn_s_barrier();                   // end of interval 2u+1
      cb = cb == 2 ? 0 : cb + 1;
    }
  } else {
    // prologue, row 1: A-hi(0), A-lo(1)
    stage_a_half(ra, lda, rows_a, 0, abuf0, 1, wc, aoff);
    if (nk > 1) stage_a_half(ra, lda, rows_a, kStep, abuf0 + kTile2Bytes, 0, wc, aoff);
    __builtin_amdgcn_s_barrier();                     // prologue barrier
    if (nk > 1) wait_vm<4>(); else wait_vm<0>();      // A-hi(0)
    __builtin_amdgcn_s_barrier();                     // end of interval 0
    int cb = 0;
    for (int u = 0; u < nk; ++u) {
      const char* ab = abuf0 + (u & 1) * kTile2Bytes;
      read_frags(ab, bbuf0 + cb * kTile2Bytes, 1);
      const bool l2 = u + 2 < nk;
      if (l2) stage_a_half(ra, lda, rows_a, (u + 2) * kStep, abuf0 + (u & 1) * kTile2Bytes, 0, wc,
                           aoff);
      if (BAL && l2) {
        const int cb2 = cb == 0 ? 2 : cb - 1;         // (u + 2) % 3
        stage_b<NBI / 2, NBI>(rb, ldb, rows_b, (u + 2) * kStep, bbuf0 + cb2 * kTile2Bytes, wc, boff);
      }
      if (u + 1 < nk) {                               // retire A-lo(u+1) (BAL: and B1(u+1))
        if (l2) { if (BAL) wait_vm<4 + NBI / 2>(); else wait_vm<4>(); }
        else wait_vm<0>();
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();                   // end of interval 2u+1
      __builtin_amdgcn_sched_barrier(0);
      mfma_all();
      __builtin_amdgcn_sched_barrier(0);
      if (u + 1 < nk) __builtin_amdgcn_s_barrier();   // end of interval 2u+2
      cb = cb == 2 ? 0 : cb + 1;
    }
  }
  store_tile(a, acc, m0 + wr * 128, n0 + wc * 64, lane);
}

__global__ void __launch_bounds__(kThreads2, 1) gemm_fp8_nt_256_pingpong3(Fp8Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  pingpong_body<false>(a, smem);
}

__global__ void __launch_bounds__(kThreads2, 1) gemm_fp8_nt_256_pingpong3_bal(Fp8Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  pingpong_body<true>(a, smem);
}

// balanced DMA issue: 0 never, 1 always, 2 = from kBalMinKTiles K-tiles on (the bf16 rule)
static int gemm_fp8_bal = 2;
constexpr int64_t kBalMinKTiles = 32;

}  // namespace fp8
}  // namespace dlbb

using namespace dlbb;
using namespace dlbb::fp8;

DLBB_API void dlbb_gemm_fp8_set_bal(int mode) { gemm_fp8_bal = mode >= 0 && mode <= 2 ? mode : 2; }

// x [M, K] bf16 (row stride ldx elements) -> q [M, K] e4m3fn (row stride ldq bytes) + scale [M].
// K % 8 == 0, K <= 16384, 16-byte aligned x rows, 8-byte aligned q rows.
DLBB_API int dlbb_quant_fp8_rows(const void* x, int64_t ldx, void* q, int64_t ldq, void* scale,
                                 int64_t M, int64_t K, hipStream_t stream) {
  if (M <= 0 || K <= 0) return hipSuccess;
  if (K % 8 || K > 16384 || ldx % 8 || ldq % 8 || ldx < K || ldq < K || !scale)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(q) & 7) ||
      (reinterpret_cast<uintptr_t>(scale) & 3))
    return hipErrorInvalidValue;
  if (M > 0x7fffffff) return hipErrorInvalidValue;
  const int K8 = static_cast<int>(K / 8);
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  uint8_t* qp = static_cast<uint8_t*>(q);
  float* sp = static_cast<float*>(scale);
  const dim3 b(kQThreads);
#define DLBB_Q_LAUNCH(WAVE_ROW, NV)                                                          \
  hipLaunchKernelGGL((quant_fp8_rows_kernel<WAVE_ROW, NV>),                                 \
                     dim3(static_cast<unsigned>(WAVE_ROW ? (M + 3) / 4 : M)), b, 0, stream, \
                     xp, ldx, qp, ldq, sp, M, K8)
  if (K8 <= 64) DLBB_Q_LAUNCH(true, 1);
  else if (K8 <= 128) DLBB_Q_LAUNCH(true, 2);
  else if (K8 <= 256) DLBB_Q_LAUNCH(true, 4);
  else if (K8 <= 512) DLBB_Q_LAUNCH(true, 8);
  else if (K8 <= 1024) DLBB_Q_LAUNCH(false, 4);
  else DLBB_Q_LAUNCH(false, 8);
#undef DLBB_Q_LAUNCH
  return hipGetLastError();
}

// C[M, N] = epilogue((A8[M, K] · B8[N, K]^T) * sa[m] * sb[n]). Contract: K % 128 == 0,
// M % 8 == 0, N % 64 == 0, 16-byte aligned rows of every operand; anything else is an error.
DLBB_API int dlbb_gemm_fp8_nt(const void* A, int64_t lda, const void* B, int64_t ldb,
                              const void* sa, const void* sb, void* C, int64_t ldc, int64_t M,
                              int64_t N, int64_t K, const void* bias, const void* residual,
                              int64_t ldr, int epi, int out_f32, hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0) return hipErrorInvalidValue;
  if (K % BK8 || M % 8 || N % 64) return hipErrorInvalidValue;
  if (lda % 16 || ldb % 16 || lda < K || ldb < K || ldc < N) return hipErrorInvalidValue;
  if (epi & ~(EPI_BIAS | EPI_GELU_ERF | EPI_GELU_TANH | EPI_RESIDUAL)) return hipErrorInvalidValue;
  if (!A || !B || !C || !sa || !sb) return hipErrorInvalidValue;
  if ((epi & EPI_BIAS) && !bias) return hipErrorInvalidValue;
  if ((epi & EPI_RESIDUAL) && (!residual || ldr % 8 || ldr < N)) return hipErrorInvalidValue;
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  if (!al16(A) || !al16(B) || !al16(C) || !al16(sb) || (reinterpret_cast<uintptr_t>(sa) & 3) ||
      ((epi & EPI_BIAS) && !al16(bias)) || ((epi & EPI_RESIDUAL) && !al16(residual)))
    return hipErrorInvalidValue;
  if (ldc % (out_f32 ? 4 : 8)) return hipErrorInvalidValue;
  // 32-bit buffer offsets within a 256-row panel
  if (lda * 256 + K >= (1LL << 31) || ldb * 256 + K >= (1LL << 31)) return hipErrorInvalidValue;
  const int64_t tiles = ((M + BM2 - 1) / BM2) * ((N + BN2 - 1) / BN2);
  if (tiles >= (1LL << 31)) return hipErrorInvalidValue;
  Fp8Args a{static_cast<const uint8_t*>(A), static_cast<const uint8_t*>(B), C,
            static_cast<const float*>(sa), static_cast<const float*>(sb),
            static_cast<const uint16_t*>(bias), static_cast<const uint16_t*>(residual),
            M, N, K, lda, ldb, ldc, ldr, epi, out_f32};
  const dim3 g(static_cast<unsigned>(tiles)), b(kThreads2);
  const bool bal = gemm_fp8_bal == 1 || (gemm_fp8_bal == 2 && K / BK8 >= kBalMinKTiles);
  if (bal) hipLaunchKernelGGL(gemm_fp8_nt_256_pingpong3_bal, g, b, kPP6Lds, stream, a);
  else hipLaunchKernelGGL(gemm_fp8_nt_256_pingpong3, g, b, kPP6Lds, stream, a);
  return hipGetLastError();
}
