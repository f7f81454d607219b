// MXFP4 (OCP MX: e2m1 codes, one e8m0 scale per 32 k) GEMM for large-M linears (ops/mxfp4.py),
// gfx950: a one-pass row quantiser and an NT GEMM with BOTH operands in MXFP4 on the block-scaled
// MFMA (v_mfma_scale_f32_16x16x128_f8f6f4 with format code 4 for both operands: 16 bytes per lane
// instead of 32, and the e8m0 scales applied inside the instruction).
//
//   quantiser: per block of 32 k: b = clamp(floor(log2 amax) - 2 + 127, 2, 254) (127 if amax == 0),
//              code = e2m1_rne(clamp(x / 2^(b-127), +-6)), sign bit set exactly when x < 0
//              (ops/mxfp4.py is the specification; the tests compare bits)
//   GEMM:      C[M,N] = epilogue( sum_k a[m,k] 2^(sa[m,k/32]-127) * b[n,k] 2^(sb[n,k/32]-127) )
//              epilogue: (+ bias[N]) -> (GELU erf | GELU tanh) -> (+ residual[M,N]) -> bf16 | fp32
//
// The GEMM is the 256 x 256, 8-wave ping-pong schedule of csrc/gemm_fp8.hip with the K-tile
// redefined once more: 256 e2m1 elements are 128 bytes, so the 128-byte tile rows, the LDS-DMA
// staging, the 16-byte-slot XOR swizzle, the permuted B rows and the 160 KiB A-double / B-triple
// plan are those of the e4m3 kernel (the staging helpers are copied here, as gemm_fp8.hip copied
// them from gemm.hip: the existing kernels keep their bits). What is new: a K-tile is two MFMA
// K-steps of 128 k (64 MFMAs per wave and K-tile), the scales travel global memory -> VGPRs (LDS
// is full), and one vmcnt(0) per memory interval replaces the counted waits of the loop.
#include <utility>

#include "common.h"

namespace dlbb {
namespace mx4 {

typedef int i32x8 __attribute__((ext_vector_type(8)));     // scaled-MFMA operand (e2m1: low half)
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

enum Epi : int { EPI_BIAS = 1, EPI_GELU_ERF = 2, EPI_GELU_TANH = 4, EPI_RESIDUAL = 8 };

// ---------------------------------------------------------------------------------------
// Row quantiser. A row is read from memory ONCE (quant_fp8_rows_kernel's plan): every thread
// keeps its NV 16-byte vectors (8 bf16 each) in registers between the block amax and the convert.
//   WAVE_ROW: one wave per row (4 rows per 256-thread workgroup), K <= 64 * 8 * NV
//   else:     one workgroup per row,                              K <= 256 * 8 * NV
// Vector c of a row covers k [8 c, 8 c + 8), so a block of 32 k is the vectors of 4 consecutive
// lanes: its amax is two xor-shuffles, no LDS. floor(log2 amax) is the exponent field of amax (a
// subnormal amax lies below every scale the clamp allows). Finite bf16 input gives b in [2, 252],
// where 1 / 2^(b-127) = 2^(127-b) is a normal fp32 and the multiply by it is exact (b = 254 would
// make it 0; inf / NaN are outside the contract); the rounding is the torch
// formula's: round-half-even on the grid step 0.5 below 2, 1 below 4, 2 above.
constexpr int kQThreads = 256;

__device__ __forceinline__ uint32_t e2m1_code(float x, float inv) {
  const float a = __builtin_fminf(__builtin_fabsf(x) * inv, 6.0f);
  const float c = a < 2.0f ? __builtin_rintf(a * 2.0f)
                           : (a < 4.0f ? __builtin_rintf(a) + 2.0f : __builtin_rintf(a * 0.5f) + 4.0f);
  return static_cast<uint32_t>(c) | (x < 0.0f ? 8u : 0u);
}

template <bool WAVE_ROW, int NV>
__global__ void __launch_bounds__(kQThreads) quant_mxfp4_rows_kernel(
    const uint16_t* __restrict__ x, int64_t ldx, uint8_t* __restrict__ codes, int64_t ldc,
    uint8_t* __restrict__ scales, int64_t lds, int64_t M, int K8) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = WAVE_ROW ? static_cast<int64_t>(blockIdx.x) * (kQThreads / kWave) + wave
                               : static_cast<int64_t>(blockIdx.x);
  const int t = WAVE_ROW ? lane : static_cast<int>(threadIdx.x);
  constexpr int kStride = WAVE_ROW ? kWave : kQThreads;
  if (row >= M) return;                            // wave-uniform
  const u16x8* xr = reinterpret_cast<const u16x8*>(x + row * ldx);
  u16x8 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = t + i * kStride;
    v[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (c < K8) v[i] = xr[c];                      // K8 % 4 == 0: uniform over a block's 4 lanes
  }
  uint32_t* cr = reinterpret_cast<uint32_t*>(codes + row * ldc);
  uint8_t* sr = scales + row * lds;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = t + i * kStride;
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = __builtin_fmaxf(amax, __builtin_fabsf(bf16_to_f32(v[i][j])));
    amax = __builtin_fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = __builtin_fmaxf(amax, __shfl_xor(amax, 2, 64));
    if (c >= K8) continue;
    const int e = static_cast<int>(__float_as_uint(amax) >> 23);
    int b = e - 2;
    b = b < 2 ? 2 : (b > 254 ? 254 : b);
    if (amax == 0.f) b = 127;
    const float inv = __uint_as_float(static_cast<uint32_t>(254 - b) << 23);
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) w |= e2m1_code(bf16_to_f32(v[i][j]), inv) << (4 * j);
    cr[c] = w;
    if ((c & 3) == 0) sr[c >> 2] = static_cast<uint8_t>(b);
  }
}

// ---------------------------------------------------------------------------------------
// GEMM. Tile geometry in BYTES (identical to the bf16 and e4m3 ping-pong: 128-byte rows).
constexpr int BM2 = 256, BN2 = 256;
constexpr int BK4 = 256;                       // K-tile in e2m1 elements
constexpr int kRowBytes = BK4 / 2;             // 128
constexpr int kThreads2 = 512;
constexpr int kTile2Bytes = BM2 * kRowBytes;   // 32 KiB per operand
constexpr int kPP6Lds = 5 * kTile2Bytes;       // A double + B triple = 160 KiB
constexpr int kGroupM = 8;
constexpr int kScaleLoads = 12;                // 16-bit scale loads per wave and K-tile (8 A + 4 B)

struct Mx4Args {
  const uint8_t* A;        // [M, K/2] e2m1 pairs, row stride lda bytes
  const uint8_t* B;        // [N, K/2] e2m1 pairs, row stride ldb bytes
  void* C;                 // [M, N] bf16 | fp32, row stride ldc elements
  const uint8_t* sa;       // [M, K/32] e8m0, row stride lds_a bytes
  const uint8_t* sb;       // [N, K/32] e8m0, row stride lds_b bytes
  const uint16_t* bias;    // [N] bf16
  const uint16_t* residual;  // [M, N] bf16, row stride ldr
  int64_t M, N, K;
  int64_t lda, ldb, ldc, ldr, lds_a, lds_b;
  int epi;
  int out_f32;
};

struct Tile256 {
  int64_t m0, n0;
};

// virtual workgroup id -> output tile: XCD-aware bijective remap, then GROUP_M ordering
__device__ __forceinline__ Tile256 tile_of(const Mx4Args& a, int vb) {
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
    bldsx4(ra, aoff, static_cast<uint32_t>(g) * lda + k0, abuf + trow * kRowBytes);
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
    bldsx4(rb, boff, static_cast<uint32_t>(g) * ldb + k0, bbuf + trow * kRowBytes);
  }
}

// One lane's operands of BOTH K-steps of a K-tile: 32 bytes of tile row `row`, the low 16 for
// step 0 and the high 16 for step 1.
// Operand and scale lane map of v_mfma_scale_f32_16x16x128_f8f6f4 with e2m1 operands, established
// on the GPU (a one-wave probe with a distinct scale byte per lane and per byte position, and
// tests/test_mxfp4_gemm_gpu.py's exact products with a different scale in every k-block): lane l
// supplies matrix row l & 15 and 32 of the instruction's 128 k in 16 bytes (the low nibble of
// byte t is element 2 t); code t of A-lane (row i, group g = l >> 4) is multiplied with code t of
// B-lane (row j, group g), so any 16-byte slice per lane group is right as long as A, B and the
// scales take the same one. The scale of a lane's 32 k comes from THAT LANE's scale VGPR — lane l
// scales row l & 15, group l >> 4, for either operand — and op_sel in {0, 1, 2, 3} selects byte
// op_sel of that VGPR. Four blocks with four different scales are summed exactly.
// The k-cut: step s, group g takes bytes [32 g + 16 s, +16) of the 128-byte row, i.e. k-block
// 8 u + 2 g + s of K-tile u — in LDS the swizzled 16-byte slots (2 g) ^ (row & 7) and that ^ 1 —
// so the two scales a lane needs per row and K-tile are adjacent bytes: one 16-bit load.
__device__ __forceinline__ i32x8 read_frag(const char* lds, int row, int fq) {
  const int off = row * kRowBytes + (((2 * fq) ^ (row & 7)) << 4);
  const i32x4 lo = *reinterpret_cast<const i32x4*>(lds + off);
  const i32x4 hi = *reinterpret_cast<const i32x4*>(lds + (off ^ 16));
  return i32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int S>
__device__ __forceinline__ i32x8 step_operand(const i32x8& f) {
  return i32x8{f[4 * S], f[4 * S + 1], f[4 * S + 2], f[4 * S + 3], 0, 0, 0, 0};
}

// MFMA T of a K-tile: K-step S, A fragment row I, B fragment row J. sc[p] holds the scale bytes
// of fragment rows 2 p (bytes 0, 1 = steps 0, 1) and 2 p + 1 (bytes 2, 3); A rows in sc[0..3],
// B rows in sc[4..5]. Operands swapped (D = W rows x X rows^T): a lane's 4 accumulator registers
// are 4 consecutive output columns. Format code 4 = e2m1 for both operands.
template <int T>
__device__ __forceinline__ void mfma_one(f32x4 (&acc)[8][4], const i32x8 (&af)[8],
                                         const i32x8 (&bf)[4], const int (&sc)[6]) {
  constexpr int S = T / 32, I = (T / 4) % 8, J = T % 4;
  acc[I][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
      step_operand<S>(bf[J]), step_operand<S>(af[I]), acc[I][J], 4, 4, 2 * (J & 1) + S,
      sc[4 + J / 2], 2 * (I & 1) + S, sc[I / 2]);
}

// the 32 MFMAs of K-step S
template <int S, int... T>
__device__ __forceinline__ void mfma_step(f32x4 (&acc)[8][4], const i32x8 (&af)[8],
                                          const i32x8 (&bf)[4], const int (&sc)[6],
                                          std::integer_sequence<int, T...>) {
  (mfma_one<32 * S + T>(acc, af, bf, sc), ...);
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
__device__ __forceinline__ void store_tile(const Mx4Args& a, const f32x4 (&acc)[8][4],
                                           int64_t row0, int64_t col0, int lane) {
  const int fr = lane & 15, fq = lane >> 4;
  const int epi = a.epi;
  const int64_t cbase = col0 + fq * 16;
  if (cbase >= a.N) return;
  const int64_t rbase = row0 + fr;
  const int rows_left = static_cast<int>(a.M - rbase);
  float bias[16];
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
    float v[16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[j * 4 + r] = acc[i][j][r] + bias[j * 4 + r];
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

// The ping-pong schedule of csrc/gemm_fp8.hip (2 wave rows x 4 wave columns, 128 x 64 outputs per
// wave; the wave rows alternate between a memory interval and an MFMA interval):
//   interval 2u   (row 0 reads tile u):  row 0 issues A-hi(u+1) and B(u+2)
//   interval 2u+1 (row 1 reads tile u):  row 1 issues A-lo(u+2)
// S(u) are a wave's own kScaleLoads scale loads of tile u (global / L2 -> VGPR, 16 bits each;
// every wave needs the scales of its 128 A rows and 64 B rows). The kernel sits at the register
// limit (128 accumulators + 96 fragment registers): 12 scale registers in flight next to live
// fragments spill, whether the loads run a K-tile ahead or through the memory interval. So a wave
// issues S(u) at the top of its memory interval of tile u, where no fragment is live, and packs
// them to 6 VGPRs before the fragment reads. That exposes one L2 round trip per K-tile in the
// memory interval, and — memory returns in order — retires the LDS-DMA the wave issued in its
// previous memory interval there: a DMA has one K-tile period to land, not two as in the e4m3
// kernel. That full drain (pack_scales: vmcnt(0)) IS the synchronisation of the loop; the
// e4m3 kernel's counted waits are gone, only the prologue keeps them. What each barrier needs, and
// the drain that gives it (a wave drains at the top of each of its memory intervals):
//   row 0 ends interval 2u with A-hi(u) retired and 2u+1 with B(u+1) retired: both were issued in
//     interval 2u-2 and drained at the top of 2u (tile 0's A-hi and B(1) come from the prologues);
//   row 1 ends 2u+1 with A-lo(u+1) (BAL: and B1(u+1)) retired: issued in 2u-1, drained at the top
//     of 2u+1.
// Every DMA for tile t is issued in an iteration before the one that reads t, so a drain follows
// it. Moving the scale loads ahead again (one K-tile, as the register budget does not allow
// today) needs the counted waits back, with the scale loads counted in. WAR: A-hi(u+1) replaces A-hi(u-1), B(u+2) replaces B(u-1) (both last read in
// interval 2u-1), A-lo(u+2) replaces A-lo(u) (row 0, 2u) — each behind the barrier that closes the
// read.
// BAL: the second half of every B tile from tile 2 on is issued by wave row 1 next to A-lo(u+2),
// so both rows issue 8 DMA instructions per K-tile; row 1 retires A-lo(u+1) and B1(u+1) together.
template <bool BAL>
__device__ __forceinline__ void pingpong_body(const Mx4Args& a, char* smem) {
  constexpr int NBI = 8;                      // B DMA instructions per staging wave per K-tile
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wave >> 2, wc = wave & 3;
  const int fr = lane & 15, fq = lane >> 4;
  const Tile256 tl = tile_of(a, static_cast<int>(blockIdx.x));
  const int64_t m0 = tl.m0, n0 = tl.n0;
  const int nk = static_cast<int>(a.K / BK4);
  char* const abuf0 = smem;
  char* const bbuf0 = smem + 2 * kTile2Bytes;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  i32x8 af[8], bf[4];
  int sc[6];                                  // packed scales of the tile being multiplied
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
  constexpr uint32_t kStep = kRowBytes;

  // Scale loads: 16-bit buffer loads, a per-lane 32-bit offset plus a wave-uniform one. A
  // fragment row i is tile row wr * 128 + 16 i + fr; a 16-row group that ragged M (M % 8 == 0)
  // cuts or drops reads the last 8 rows of the matrix instead (its live rows, if any, are exactly
  // those; the rest is masked in store_tile). B fragment row j is LDS row wc * 64 + 16 j + fr =
  // output column wc * 64 + 4 j + perm_brow(fr); a 64-column block past ragged N reads block 0, as
  // its DMA does.
  const uint32_t lsa = static_cast<uint32_t>(a.lds_a), lsb = static_cast<uint32_t>(a.lds_b);
  const uint32_t sa_full = static_cast<uint32_t>(fr) * lsa + 2 * fq;
  const uint32_t sa_cut = static_cast<uint32_t>(fr & 7) * lsa + 2 * fq;
  const uint32_t sb_off = static_cast<uint32_t>(perm_brow(fr)) * lsb + 2 * fq;
  const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(a.sa + m0 * a.lds_a), 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(a.sb + (n0 + (wc * 64 < rows_b ? wc * 64 : 0)) * a.lds_b), 0,
      0x7fffffff, 0x00020000);
  int raw[kScaleLoads];
  auto load_scales = [&](int u) {                                // kScaleLoads loads
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r0 = wr * 128 + i * 16;
      const bool full = r0 + 16 <= rows_a;                       // wave-uniform
      raw[i] = __builtin_amdgcn_raw_buffer_load_b16(
          rsa, full ? sa_full : sa_cut, static_cast<uint32_t>(full ? r0 : rows_a - 8) * lsa + 8 * u,
          0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      raw[8 + j] = __builtin_amdgcn_raw_buffer_load_b16(rsb, sb_off, 4 * j * lsb + 8 * u, 0);
  };
  // vmcnt(0): the scale loads just issued and, memory returning in order, every LDS-DMA of this
  // wave's previous memory interval (the loop's only DMA wait). Then two fragment rows per VGPR
  // (mfma_one).
  auto pack_scales = [&]() {
    wait_vm<0>();
#pragma unroll
    for (int p = 0; p < 6; ++p) sc[p] = raw[2 * p] | (raw[2 * p + 1] << 16);
  };

  auto read_frags = [&](const char* ab, const char* bb, int row) {
#pragma unroll
    for (int i = 0; i < 8; ++i) af[i] = read_frag(ab, row * 128 + i * 16 + fr, fq);
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = read_frag(bb, wc * 64 + j * 16 + fr, fq);
  };
  auto mfma_all = [&]() {
    mfma_step<0>(acc, af, bf, sc, std::make_integer_sequence<int, 32>{});
    mfma_step<1>(acc, af, bf, sc, std::make_integer_sequence<int, 32>{});
    // the MFMAs touch no memory, so nothing else keeps the compiler from sinking them below the
    // barrier that closes their interval: tie every accumulator to an empty
    // volatile asm, which stays in order with the barriers
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) tr_tie(acc[i][j]);
  };

  using T = std::true_type;
  using F = std::false_type;
  int cb = 0;                                         // B buffer of tile u
  // one K-tile of wave row 0; H1: tile u + 1 exists, B2: tile u + 2 exists (compile-time: the
  // steady-state loop has no branches)
  auto row0_tile = [&](auto H1, auto B2, int u) {
    constexpr bool h1 = decltype(H1)::value, b2 = decltype(B2)::value;
    const char* ab = abuf0 + (u & 1) * kTile2Bytes;
    load_scales(u);
    pack_scales();
    read_frags(ab, bbuf0 + cb * kTile2Bytes, 0);
    if constexpr (h1)
      stage_a_half(ra, lda, rows_a, (u + 1) * kStep, abuf0 + ((u + 1) & 1) * kTile2Bytes, 1, wc,
                   aoff);
    if constexpr (b2) {
      const int cb2 = cb == 0 ? 2 : cb - 1;           // (u + 2) % 3
      stage_b<0, BAL ? NBI / 2 : NBI>(rb, ldb, rows_b, (u + 2) * kStep, bbuf0 + cb2 * kTile2Bytes,
                                      wc, boff);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();                     // end of interval 2u
    __builtin_amdgcn_sched_barrier(0);
    mfma_all();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();                     // end of interval 2u+1
    cb = cb == 2 ? 0 : cb + 1;
  };
  auto row1_tile = [&](auto H1, auto L2, int u) {
    constexpr bool h1 = decltype(H1)::value, l2 = decltype(L2)::value;
    const char* ab = abuf0 + (u & 1) * kTile2Bytes;
    load_scales(u);
    pack_scales();
    read_frags(ab, bbuf0 + cb * kTile2Bytes, 1);
    if constexpr (l2)
      stage_a_half(ra, lda, rows_a, (u + 2) * kStep, abuf0 + (u & 1) * kTile2Bytes, 0, wc, aoff);
    if constexpr (BAL && l2) {
      const int cb2 = cb == 0 ? 2 : cb - 1;           // (u + 2) % 3
      stage_b<NBI / 2, NBI>(rb, ldb, rows_b, (u + 2) * kStep, bbuf0 + cb2 * kTile2Bytes, wc, boff);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();                     // end of interval 2u+1
    __builtin_amdgcn_sched_barrier(0);
    mfma_all();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (h1) __builtin_amdgcn_s_barrier();   // end of interval 2u+2
    cb = cb == 2 ? 0 : cb + 1;
  };

  int u = 0;
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
    for (; u + 2 < nk; ++u) row0_tile(T{}, T{}, u);
    if (u + 1 < nk) row0_tile(T{}, F{}, u++);
    row0_tile(F{}, F{}, u);
  } else {
    // prologue, row 1: A-hi(0), A-lo(1)
    stage_a_half(ra, lda, rows_a, 0, abuf0, 1, wc, aoff);
    if (nk > 1) stage_a_half(ra, lda, rows_a, kStep, abuf0 + kTile2Bytes, 0, wc, aoff);
    __builtin_amdgcn_s_barrier();                     // prologue barrier
    if (nk > 1) wait_vm<4>(); else wait_vm<0>();      // A-hi(0)
    __builtin_amdgcn_s_barrier();                     // end of interval 0
    for (; u + 2 < nk; ++u) row1_tile(T{}, T{}, u);
    if (u + 1 < nk) row1_tile(T{}, F{}, u++);
    row1_tile(F{}, F{}, u);
  }
  store_tile(a, acc, m0 + wr * 128, n0 + wc * 64, lane);
}

__global__ void __launch_bounds__(kThreads2, 1) gemm_mxfp4_nt_256_pingpong3(Mx4Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  pingpong_body<false>(a, smem);
}

__global__ void __launch_bounds__(kThreads2, 1) gemm_mxfp4_nt_256_pingpong3_bal(Mx4Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  pingpong_body<true>(a, smem);
}

constexpr int64_t kBalMinKTiles = 32;          // balanced DMA issue from K = 8192 on (the FP8 rule)

}  // namespace mx4
}  // namespace dlbb

using namespace dlbb;
using namespace dlbb::mx4;

// x [M, K] bf16 (row stride ldx elements) -> codes [M, K/2] (row stride ldc bytes; low nibble =
// even k) + scales [M, K/32] e8m0 (row stride lds bytes). K % 32 == 0, K <= 16384, 16-byte
// aligned x rows, 4-byte aligned code rows.
DLBB_API int dlbb_quant_mxfp4_rows(const void* x, int64_t ldx, void* codes, int64_t ldc,
                                   void* scales, int64_t lds, int64_t M, int64_t K,
                                   hipStream_t stream) {
  if (M <= 0 || K <= 0) return hipSuccess;
  if (K % 32 || K > 16384 || ldx % 8 || ldx < K || ldc % 4 || ldc < K / 2 || lds < K / 32)
    return hipErrorInvalidValue;
  if (!x || !codes || !scales || (reinterpret_cast<uintptr_t>(x) & 15) ||
      (reinterpret_cast<uintptr_t>(codes) & 3))
    return hipErrorInvalidValue;
  if (M > 0x7fffffff) return hipErrorInvalidValue;
  const int K8 = static_cast<int>(K / 8);
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  uint8_t* cp = static_cast<uint8_t*>(codes);
  uint8_t* sp = static_cast<uint8_t*>(scales);
  const dim3 b(kQThreads);
#define DLBB_Q4_LAUNCH(WAVE_ROW, NV)                                                         \
  hipLaunchKernelGGL((quant_mxfp4_rows_kernel<WAVE_ROW, NV>),                               \
                     dim3(static_cast<unsigned>(WAVE_ROW ? (M + 3) / 4 : M)), b, 0, stream, \
                     xp, ldx, cp, ldc, sp, lds, M, K8)
  if (K8 <= 64) DLBB_Q4_LAUNCH(true, 1);
  else if (K8 <= 128) DLBB_Q4_LAUNCH(true, 2);
  else if (K8 <= 256) DLBB_Q4_LAUNCH(true, 4);
  else if (K8 <= 512) DLBB_Q4_LAUNCH(true, 8);
  else if (K8 <= 1024) DLBB_Q4_LAUNCH(false, 4);
  else DLBB_Q4_LAUNCH(false, 8);
#undef DLBB_Q4_LAUNCH
  return hipGetLastError();
}

// C[M, N] = epilogue(sum_k a 2^(sa-127) * b 2^(sb-127)). Contract: K % 256 == 0, M % 8 == 0,
// N % 64 == 0, 16-byte aligned rows of A, B, C (lda, ldb >= K/2 bytes), 8-byte aligned scale rows
// (lds_a, lds_b >= K/32); anything else is an error and launches nothing.
DLBB_API int dlbb_gemm_mxfp4_nt(const void* A, int64_t lda, const void* sa, int64_t lds_a,
                                const void* B, int64_t ldb, const void* sb, int64_t lds_b, void* C,
                                int64_t ldc, int64_t M, int64_t N, int64_t K, const void* bias,
                                const void* residual, int64_t ldr, int epi, int out_f32,
                                hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0) return hipErrorInvalidValue;
  if (K % BK4 || M % 8 || N % 64) return hipErrorInvalidValue;
  if (lda % 16 || ldb % 16 || lda < K / 2 || ldb < K / 2 || ldc < N) return hipErrorInvalidValue;
  if (lds_a % 8 || lds_b % 8 || lds_a < K / 32 || lds_b < K / 32) return hipErrorInvalidValue;
  if (epi & ~(EPI_BIAS | EPI_GELU_ERF | EPI_GELU_TANH | EPI_RESIDUAL)) return hipErrorInvalidValue;
  if (!A || !B || !C || !sa || !sb) return hipErrorInvalidValue;
  if ((epi & EPI_BIAS) && !bias) return hipErrorInvalidValue;
  if ((epi & EPI_RESIDUAL) && (!residual || ldr % 8 || ldr < N)) return hipErrorInvalidValue;
  auto al = [](const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; };
  if (!al(A, 16) || !al(B, 16) || !al(C, 16) || !al(sa, 8) || !al(sb, 8) ||
      ((epi & EPI_BIAS) && !al(bias, 16)) || ((epi & EPI_RESIDUAL) && !al(residual, 16)))
    return hipErrorInvalidValue;
  if (ldc % (out_f32 ? 4 : 8)) return hipErrorInvalidValue;
  // 32-bit offsets within a 256-row panel (codes and scales)
  if (lda * 256 + K >= (1LL << 31) || ldb * 256 + K >= (1LL << 31) ||
      lds_a * 256 + K >= (1LL << 31) || lds_b * 256 + K >= (1LL << 31))
    return hipErrorInvalidValue;
  const int64_t tiles = ((M + BM2 - 1) / BM2) * ((N + BN2 - 1) / BN2);
  if (tiles >= (1LL << 31)) return hipErrorInvalidValue;
  Mx4Args a{static_cast<const uint8_t*>(A), static_cast<const uint8_t*>(B), C,
            static_cast<const uint8_t*>(sa), static_cast<const uint8_t*>(sb),
            static_cast<const uint16_t*>(bias), static_cast<const uint16_t*>(residual),
            M, N, K, lda, ldb, ldc, ldr, lds_a, lds_b, epi, out_f32};
  const dim3 g(static_cast<unsigned>(tiles)), b(kThreads2);
  if (K / BK4 >= kBalMinKTiles)
    hipLaunchKernelGGL(gemm_mxfp4_nt_256_pingpong3_bal, g, b, kPP6Lds, stream, a);
  else
    hipLaunchKernelGGL(gemm_mxfp4_nt_256_pingpong3, g, b, kPP6Lds, stream, a);
  return hipGetLastError();
}
