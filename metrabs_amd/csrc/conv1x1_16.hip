// K13h: K13 (conv1x1.hip) for f16 / bf16 tensors -- a 1x1 stride-1 NCHW convolution as one 16-bit MFMA
// GEMM with the K10 epilogue and the squeeze-excite gate folded in.
//
// Not part of the reference's hot path (like K10 - K13): the expand and project convolutions of the
// backbone's 16-bit inference copy (backbones.fold_batchnorm(fused_epilogue=True, dtype=f16 / bf16)).
// PyTorch-ROCm runs each as a rocBLAS 16-bit GEMM, then K10, and the project conv behind a separate
// "x * gate" pass.  Here, per image b, in one launch:
//
//   xg[b, k, p] = x[b, k, p]                                    (no gate)
//               = rnd16(f32(x[b, k, p]) * f32(rnd16(gate[b, k])))  (torch's x * gate.to(x.dtype), bit for bit)
//   y[b, m, p]  = rnd16(act(bias[m] + sum_k W[m, k] * xg[b, k, p]) (+ residual[b, m, p]))
//
// accumulated in f32, the epilogue in f32 in K10's order, rounded to 16 bits once (round to nearest even,
// plain casts).  The GEMM is computed transposed, Y_b^T = X_b^T W^T, on v_mfma_f32_32x32x16_{f16,bf16}:
// the A operand is a 32 (positions) x 16 (k) slice of X^T, the B operand a 16 (k) x 32 (channels) slice of
// W^T.  Lane (r, h) = (lane & 31, lane >> 5) holds A[r][8h .. 8h+7] and B[8h .. 8h+7][r]: eight CONSECUTIVE
// k of one position and of one weight row.  W is row-major [M][K], so its fragment is one 16-byte load
// straight from global memory (L2-resident; each wave owns its rows, nothing to share through LDS).  X is
// k-strided (NCHW): a k-tile is staged global -> registers -> LDS as an X^T image ([position][k], rows
// padded so that the 16-byte fragment reads of 16 consecutive positions hit distinct banks), transposed on
// the way in -- each loader thread reads 4 k-rows x 8 positions (four 16-byte loads) and writes 8 positions
// x 4 k (eight 8-byte LDS writes).  Every lane of the accumulator holds four consecutive positions of one
// output channel: one 8-byte store per group, the epilogue applied in registers on the way out.
//
// The column index runs over (image, position) jointly like K13's; HW % 8 == 0, so a loader group of 8
// positions never straddles two images.  Two LDS buffers (the next tile's loads are in flight while the
// current one is multiplied); rows past M, columns past B * HW and k past K are zero-filled, never stored.
// The k order is the same in every configuration -- 16-k MFMA steps at 0, 16, 32, ... -- so the result
// does not depend on the tile picked.  No atomics, no split-K: the same inputs give the same bits.
#include <type_traits>

#include "common.h"

namespace mtr {

typedef float c16_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

template <int DT> struct Bits16;
template <> struct Bits16<MTR_F16> {
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ float f32(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
  static __device__ __forceinline__ c16_f32x16 mfma(uint4 a, uint4 b, c16_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};
template <> struct Bits16<MTR_BF16> {
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ float f32(unsigned short b) { return (float)__builtin_bit_cast(__bf16, b); }
  // a plain cast: v_cvt_pk_bf16_f32, round to nearest even, a NaN stays a NaN
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
  static __device__ __forceinline__ c16_f32x16 mfma(uint4 a, uint4 b, c16_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};

constexpr int kC16Pad = 8;  // X^T image row pad (16-bit elements): rows (BK + 8) * 2 bytes apart

// WM x WN waves, each FM x FN tiles of 32 x 32 (channels x positions), k-tiles of BK
template <int DT, int WM, int WN, int FM, int FN, int BK>
__global__ __launch_bounds__(64 * WM * WN) void conv1x1_16_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ gate, const unsigned short* __restrict__ residual, unsigned short* __restrict__ y,
    int M, int K, int HW, int n_total, FastDiv by_hw, int act) {
  using H = Bits16<DT>;
  constexpr int NT = 64 * WM * WN;
  constexpr int BM = 32 * FM * WM, BN = 32 * FN * WN;
  constexpr int LDK = BK + kC16Pad;           // elements per X^T image row (one position)
  constexpr int KS = BK / 16;                 // MFMA k-steps per tile
  constexpr int UNITS = (BK / 4) * (BN / 8);  // loader units of 4 k x 8 positions
  static_assert(BK % 16 == 0 && UNITS <= NT, "one loader unit per thread at most");
  __shared__ __attribute__((aligned(16))) unsigned short xs[2][BN * LDK];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int r = lane & 31, h = lane >> 5;

  // this thread's loader unit: positions 8 p8 .. 8 p8 + 7 of the tile, k 4 k4 .. 4 k4 + 3 of each k-tile
  const int p8 = tid % (BN / 8), k4 = tid / (BN / 8);
  const int xcol = n0 + 8 * p8;
  const bool xload = tid < UNITS && xcol < n_total;
  const unsigned xb = xload ? fastdiv((unsigned)xcol, by_hw) : 0u;
  const unsigned short* xsrc = x + (long long)xb * K * HW + (xcol - (int)xb * HW);
  const float* gsrc = gate ? gate + (long long)xb * K : nullptr;

  // the next tile's x rows and gate values: loaded in load_x, first used in store_x (behind this tile's
  // MFMAs), so the loads stay in flight while the current tile is multiplied
  u16x8 xr[4];
  float gr[4];
  auto load_x = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + 4 * k4 + i;
      u16x8 t = (u16x8)0;
      float g = 0.0f;
      if (xload && k < K) {
        t = __builtin_bit_cast(u16x8, *reinterpret_cast<const uint4*>(xsrc + (long long)k * HW));
        if (gsrc) g = gsrc[k];
      }
      xr[i] = t;
      gr[i] = g;
    }
  };
  auto store_x = [&](int buf) {  // 4 k-rows x 8 positions -> 8 positions x 4 k of the X^T image
    if (tid < UNITS) {
      if (gsrc) {  // the squeeze-excite gate, once per staged element, rounded as torch's x * gate.to(x.dtype)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float g = H::f32(H::rnd(gr[i]));
#pragma unroll
          for (int e = 0; e < 8; ++e) xr[i][e] = H::rnd(H::f32(xr[i][e]) * g);
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        uint2 v;
        v.x = (unsigned)xr[0][j] | ((unsigned)xr[1][j] << 16);
        v.y = (unsigned)xr[2][j] | ((unsigned)xr[3][j] << 16);
        *reinterpret_cast<uint2*>(&xs[buf][(8 * p8 + j) * LDK + 4 * k4]) = v;
      }
    }
  };
  // this lane's weight fragments: rows m0 + wm * 32 FM + 32 i + r, k 16 s + 8 h .. + 7 of each k-tile
  auto load_w = [&](uint4 (&wr)[FM][KS], int k0) {
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int m = m0 + wm * (32 * FM) + 32 * i + r;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int k = k0 + 16 * s + 8 * h;
        uint4 t = make_uint4(0u, 0u, 0u, 0u);
        if (m < M && k < K) t = *reinterpret_cast<const uint4*>(w + (long long)m * K + k);
        wr[i][s] = t;
      }
    }
  };

  c16_f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  uint4 wc[FM][KS], wnx[FM][KS];
  const int n_tiles = (K + BK - 1) / BK;
  load_x(0);
  load_w(wc, 0);
  store_x(0);
  __syncthreads();
  for (int t = 0; t < n_tiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < n_tiles) {  // in flight during this tile's MFMAs
      load_x((t + 1) * BK);
      load_w(wnx, (t + 1) * BK);
    }
    const unsigned short* xa = &xs[buf][(wn * (32 * FN) + r) * LDK + 8 * h];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      uint4 a[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) a[j] = *reinterpret_cast<const uint4*>(xa + (32 * j) * LDK + 16 * s);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = H::mfma(a[j], wc[i][s], acc[i][j]);
    }
    if (t + 1 < n_tiles) {
      store_x(buf ^ 1);  // the other buffer: last read before the previous barrier
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int s = 0; s < KS; ++s) wc[i][s] = wnx[i][s];
    }
    __syncthreads();
  }

  // epilogue: lane holds channel m = .. + r, positions 8 g + 4 h + 0..3 of each 32-column tile
  auto epilogue = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int m = m0 + wm * (32 * FM) + 32 * i + r;
      if (m >= M) continue;
      const float bm = bias[m];
#pragma unroll
      for (int j = 0; j < FN; ++j) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = n0 + wn * (32 * FN) + 32 * j + 8 * g + 4 * h;
          if (col >= n_total) continue;
          const unsigned b = fastdiv((unsigned)col, by_hw);
          const long long off = ((long long)b * M + m) * HW + (col - (int)b * HW);
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = activate<ACT>(acc[i][j][4 * g + e] + bm);
          if (residual) {  // the block's skip connection, added after the activation (K10's order)
            const uint2 q = *reinterpret_cast<const uint2*>(residual + off);
            v[0] += H::f32((unsigned short)(q.x & 0xffffu));
            v[1] += H::f32((unsigned short)(q.x >> 16));
            v[2] += H::f32((unsigned short)(q.y & 0xffffu));
            v[3] += H::f32((unsigned short)(q.y >> 16));
          }
          uint2 o;
          o.x = (unsigned)H::rnd(v[0]) | ((unsigned)H::rnd(v[1]) << 16);
          o.y = (unsigned)H::rnd(v[2]) | ((unsigned)H::rnd(v[3]) << 16);
          *reinterpret_cast<uint2*>(y + off) = o;
        }
      }
    }
  };
  // wave-uniform: one epilogue body per activation, the GEMM shared.  Written out: behind the shared with_act() the
  // compiler forms the epilogue's column indices another way, four instructions more
  switch (act) {
    case kActRelu: epilogue(ActTag<kActRelu>()); break;
    case kActSilu: epilogue(ActTag<kActSilu>()); break;
    case kActHardswish: epilogue(ActTag<kActHardswish>()); break;
    default: epilogue(ActTag<kActNone>()); break;
  }
}

// The deep-K configuration: a few hundred output channels behind a long k loop (the project convolutions of
// the MBConv tails: K = 768 .. 3840).  The tiles above keep ONE k-tile of global loads in flight and read W
// from L2 per wave; the 128 x 128 tiles leave half the CUs idle on 12x12 maps.  Here a workgroup of four
// waves takes 64 channels x 64 columns, every wave one 32 x 32 tile -- a single accumulation chain of the
// 32x32x16 MFMA issues back to back, so one chain per wave costs no throughput -- which gives 2 - 3 workgroups
// per CU on those shapes.  k-tiles of 64 go global -> registers -> a ring of three LDS stages like K13's
// deep-K: tile t + 3 is requested before tile t is multiplied and tile t + 2 (requested one whole tile
// earlier) is written to LDS between the two halves of tile t's MFMAs.  Waves 0 and 1 stage x (transposed
// into the X^T image as above, the gate product on the way), waves 2 and 3 stage W as it lies in memory
// ([m][k], rows padded like the X^T image), so both MFMA operands are 16-byte LDS reads and W crosses L2
// once per workgroup.  The loads carry no condition: walked pointers over the whole tiles, clamped addresses in the
// tail, zero-fill on the way to LDS.  The
// accumulators leave through LDS ([channel][position] f32), so every store instruction writes 128-byte row
// segments and the residual is read the same way.  The same 16-k MFMA steps in the same order as every
// other configuration, and the same epilogue expression: the same bits.
constexpr int kDk16BM = 64, kDk16BN = 64, kDk16BK = 64, kDk16Stages = 3;
constexpr int kDk16LDK = kDk16BK + kC16Pad;  // elements per row of the X^T and W images
constexpr int kDk16LDY = kDk16BN + 4;        // floats per channel row of the staged result

template <int DT, bool GATE>
__global__ __launch_bounds__(256) void conv1x1_16_deepk_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ gate, const unsigned short* __restrict__ residual, unsigned short* __restrict__ y,
    int M, int K, int HW, int n_total, FastDiv by_hw, int act) {
  using H = Bits16<DT>;
  constexpr int BM = kDk16BM, BN = kDk16BN, BK = kDk16BK, LDK = kDk16LDK, LDY = kDk16LDY;
  constexpr int XS = BN * LDK, WS = BM * LDK;  // elements per stage
  static_assert((BK / 4) * (BN / 8) == 128 && BM * (BK / 8) == 4 * 128, "loader mappings: 128 threads each");
  static_assert(BM * LDY * 4 <= kDk16Stages * (XS + WS) * 2, "the staged result fits the ring");
  __shared__ __attribute__((aligned(16))) unsigned short lds[kDk16Stages * (XS + WS)];
  unsigned short* xs = lds;                     // [stage][position][LDK]
  unsigned short* ws = lds + kDk16Stages * XS;  // [stage][channel][LDK]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int r = lane & 31, h = lane >> 5;

  // loader roles, fixed for the whole k loop (wave-uniform).  x: positions 8 p8 .. + 7, k 4 q + i of each k-tile
  // (a wave takes 32 k: a load instruction reads whole 128-byte rows, and the 8-byte LDS writes of 16 lanes -- eight
  // q, two p8 -- are two-way on a bank at most); W: rows q + 16 i, k 8 p8 .. + 7.  Either way four 16-byte loads at
  // src[i] + min(k0 + kb + i * ki, kmax) * kmul.
  const bool isx = __builtin_amdgcn_readfirstlane(tid) < 128;
  const int p8 = isx ? (tid >> 3) & 7 : tid & 7, q = isx ? (tid & 7) | ((tid >> 6) & 1) << 3 : (tid & 127) >> 3;
  const int xcol = n0 + 8 * p8;
  const bool xcol_ok = xcol < n_total;
  const unsigned xb = xcol_ok ? fastdiv((unsigned)xcol, by_hw) : 0u;
  const unsigned short* src[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    src[i] = isx ? x + (long long)xb * K * HW + (xcol_ok ? xcol - (int)xb * HW : 0)
                 : w + (long long)min(m0 + q + 16 * i, M - 1) * K;
  const int kb = isx ? 4 * q : 8 * p8, ki = isx ? 1 : 0, kmax = isx ? K - 1 : K - 8, kmul = isx ? HW : 1;
  // the gate of the x rows; the W waves read bias[0] instead (any readable float: never used)
  const float* gsrc = GATE && isx ? gate + (long long)xb * K : bias;
  const int gmul = GATE && isx ? 1 : 0;
  // the main loop's loads (whole tiles: nothing to clamp) walk pointers, tile 3 first; the W waves' "gate" there is
  // the gate row of their own column and k group, in bounds like the x waves' and as unused as bias[0]
  const unsigned short* cur[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) cur[i] = src[i] + (long long)(3 * BK + kb + i * ki) * kmul;
  const float* gcur = GATE ? gate + (long long)xb * K + 3 * BK + 4 * q : bias;  // (q < 16 in both roles)
  const long long adv = (long long)BK * kmul;

  // Two register sets (tiles t + 2 and t + 3 are in flight together), always indexed by a constant.
  uint4 rr[2][4];
  float rg[2][4];
  auto load_tile = [&](int kt, auto set) {
    constexpr int P = decltype(set)::value;
    const int k0 = kt * BK + kb;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = min(k0 + i * ki, kmax);
      rr[P][i] = *reinterpret_cast<const uint4*>(src[i] + k * kmul);
      if constexpr (GATE) rg[P][i] = gsrc[k * gmul];
    }
  };
  auto load_next_whole_tile = [&](auto set) {
    constexpr int P = decltype(set)::value;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      rr[P][i] = *reinterpret_cast<const uint4*>(cur[i]);
      if constexpr (GATE) rg[P][i] = gcur[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) cur[i] += adv;
    if constexpr (GATE) gcur += BK;
  };
  auto store_tile = [&](int stage, int kt, auto set) {
    constexpr int P = decltype(set)::value;
    const int k0 = kt * BK + kb;
    if (isx) {  // 4 k-rows x 8 positions -> 8 positions x 4 k of the X^T image
      u16x8 xr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xr[i] = __builtin_bit_cast(u16x8, rr[P][i]);
        if constexpr (GATE) {  // the squeeze-excite gate, once per staged element, rounded as torch's x * gate.to(x.dtype)
          const float g = H::f32(H::rnd(rg[P][i]));
#pragma unroll
          for (int e = 0; e < 8; ++e) xr[i][e] = H::rnd(H::f32(xr[i][e]) * g);
        }
        const bool ok = xcol_ok && k0 + i < K;  // (a clamped load may give anything: selected away, never multiplied to zero)
#pragma unroll
        for (int e = 0; e < 8; ++e) xr[i][e] = ok ? xr[i][e] : (unsigned short)0;
      }
      unsigned short* xd = &xs[stage * XS + (8 * p8) * LDK + 4 * q];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        uint2 v;
        v.x = (unsigned)xr[0][j] | ((unsigned)xr[1][j] << 16);
        v.y = (unsigned)xr[2][j] | ((unsigned)xr[3][j] << 16);
        *reinterpret_cast<uint2*>(xd + j * LDK) = v;
      }
    } else {
      // (the gate registers count as read on this path too: a load left pending here makes the wait-count pass hold
      // the next load into the same register back until most of the tile in flight has arrived)
      if constexpr (GATE) asm volatile("" ::"v"(rg[P][0]), "v"(rg[P][1]), "v"(rg[P][2]), "v"(rg[P][3]));
      const bool k_ok = k0 < K;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = k_ok && m0 + q + 16 * i < M;
        uint4 u = rr[P][i];
        u.x = ok ? u.x : 0u; u.y = ok ? u.y : 0u; u.z = ok ? u.z : 0u; u.w = ok ? u.w : 0u;
        *reinterpret_cast<uint4*>(&ws[stage * WS + (q + 16 * i) * LDK + 8 * p8]) = u;
      }
    }
  };

  c16_f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
  auto multiply = [&](int stage, int s0) {
    const unsigned short* xa = &xs[stage * XS + (wn * 32 + r) * LDK + 8 * h];
    const unsigned short* wa = &ws[stage * WS + (wm * 32 + r) * LDK + 8 * h];
#pragma unroll
    for (int s = s0; s < s0 + BK / 32; ++s)
      acc = H::mfma(*reinterpret_cast<const uint4*>(xa + 16 * s), *reinterpret_cast<const uint4*>(wa + 16 * s), acc);
  };

  const int n_tiles = (K + BK - 1) / BK;
  constexpr std::integral_constant<int, 0> ra{};
  constexpr std::integral_constant<int, 1> rb{};
  load_tile(0, ra);
  if (n_tiles > 1) load_tile(1, rb);
  store_tile(0, 0, ra);
  if (n_tiles > 1) store_tile(1, 1, rb);
  if (n_tiles > 2) load_tile(2, ra);
  __syncthreads();
  // at the top of step t: tiles t and t + 1 are in LDS, tile t + 2 is on its way to `hold`
  int stage = 0;
  auto step = [&](int t, auto hold, auto issue, auto guarded) {
    constexpr bool G = decltype(guarded)::value;
    if constexpr (!G) load_next_whole_tile(issue);
    else if (t + 3 < n_tiles) load_tile(t + 3, issue);
    multiply(stage, 0);
    __builtin_amdgcn_sched_barrier(0);
    // stage of tile t + 2 = stage of tile t - 1: last read before the previous barrier
    if (!G || t + 2 < n_tiles) store_tile(stage == 0 ? 2 : stage - 1, t + 2, hold);
    __builtin_amdgcn_sched_barrier(0);
    multiply(stage, BK / 32);
    stage = stage == 2 ? 0 : stage + 1;
    __syncthreads();
  };
  // the body of the loop has no condition around its loads; the last steps, which have, run apart
  int t = 0;
  for (; t + 5 < n_tiles; t += 2) {  // tiles t + 3 and t + 4 are whole: neither is the last one
    step(t, ra, rb, std::false_type{});
    step(t + 1, rb, ra, std::false_type{});
  }
  for (; t < n_tiles; t += 2) {
    step(t, ra, rb, std::true_type{});
    if (t + 1 < n_tiles) step(t + 1, rb, ra, std::true_type{});
  }

  // the ring is free (the barrier above): the lane's channel wm 32 + r, positions wn 32 + 8 g + 4 h + 0..3
  float* ys = reinterpret_cast<float*>(lds);  // [channel][LDY]
#pragma unroll
  for (int g = 0; g < 4; ++g)
    *reinterpret_cast<float4*>(&ys[(wm * 32 + r) * LDY + wn * 32 + 8 * g + 4 * h]) =
        make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
  __syncthreads();
  // eight threads per channel row: 8 positions (16 bytes of y and of the residual) each
  auto epilogue = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
#pragma unroll
    for (int u = 0; u < BM * (BN / 8) / 256; ++u) {
      const int ch = (tid >> 3) + 32 * u, c8 = 8 * (tid & 7), m = m0 + ch, col = n0 + c8;
      if (m >= M || col >= n_total) continue;
      const float bm = bias[m];
      const unsigned b = fastdiv((unsigned)col, by_hw);
      const long long off = ((long long)b * M + m) * HW + (col - (int)b * HW);
      const float4 a0 = *reinterpret_cast<const float4*>(&ys[ch * LDY + c8]);
      const float4 a1 = *reinterpret_cast<const float4*>(&ys[ch * LDY + c8 + 4]);
      float v[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = activate<ACT>(v[e] + bm);
      if (residual) {  // the block's skip connection, added after the activation (K10's order)
        const u16x8 q8 = __builtin_bit_cast(u16x8, *reinterpret_cast<const uint4*>(residual + off));
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += H::f32(q8[e]);
      }
      u16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = H::rnd(v[e]);
      *reinterpret_cast<uint4*>(y + off) = __builtin_bit_cast(uint4, o);
    }
  };
  with_act(act, epilogue);
}

// The tile table, chosen from the shape only:
//   tall  (WM w, WN 1, FM 1, FN 1, BK 64): 32 w x 32, w = ceil(M / 32) <= 5 -- few output channels (the
//          project convs): the whole of M in one workgroup, every position read once
//   tall4 at M = 256, K >= 512 (8x8 projects): two workgroups of 4 waves per 32 columns
//   square(WM 2, WN 2, FM 2, FN 2, BK 32): 128 x 128 -- many output channels (expand, head)
//   deepk (2 x 2 waves of one 32 x 32 tile, BK 64 in a ring of three): 64 x 64 -- a few hundred output channels
//          behind a long k loop (conv1x1_16_deepk_kernel above); never the library's own choice, asked for by
//          mtr_conv1x1_bias_act16_opts
enum Conv1x1Config16 { kCfg16Tall = 0, kCfg16Square = 1, kCfg16DeepK = 2 };

struct Conv1x1Plan16 { int cfg, waves_m; };

inline Conv1x1Plan16 pick_config16(int M, int K) {
  if (M <= 160) return {kCfg16Tall, (M + 31) / 32};
  if (M == 256 && K >= 512) return {kCfg16Tall, 4};
  return {kCfg16Square, 2};
}

// config: -1 the library's own choice, else a Conv1x1Config16 forced on the shape (every one takes every shape; tall
// past 160 channels as rows of 128-channel workgroups)
inline int plan_for16(int M, int K, int config, Conv1x1Plan16* p) {
  switch (config) {
    case -1: *p = pick_config16(M, K); return MTR_OK;
    case kCfg16Tall: *p = {kCfg16Tall, M <= 160 ? (M + 31) / 32 : 4}; return MTR_OK;
    case kCfg16Square: *p = {kCfg16Square, 2}; return MTR_OK;
    case kCfg16DeepK: *p = {kCfg16DeepK, kDk16BM / 32}; return MTR_OK;
    default: return MTR_E_PARAM;
  }
}

// One K13h launch's arguments, as the entry point has checked them
struct Conv1x1Args16 {
  const unsigned short *x, *w;
  const float *bias, *gate;
  const unsigned short* residual;
  unsigned short* y;
  int act, M, K, HW;
  long long n_total;
  hipStream_t stream;
};

// Launches `kern` on a grid of bm-channel x bn-column tiles
template <typename Kern>
static int launch_conv1x1_16(Kern kern, const Conv1x1Args16& a, int bm, int bn, int threads) {
  const long long gx = (a.n_total + bn - 1) / bn, gy = (a.M + bm - 1) / bm;
  if (gx > 0x7fffffffLL || gy > 65535) return MTR_E_SHAPE;
  MTR_CLEAR_STALE();
  hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(threads), 0, a.stream, a.x, a.w, a.bias, a.gate,
                     a.residual, a.y, a.M, a.K, a.HW, (int)a.n_total, make_fastdiv((unsigned)a.HW), a.act);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

template <int DT, int WM, int WN, int FM, int FN, int BK>
static int launch_tiles16(const Conv1x1Args16& a) {
  return launch_conv1x1_16(conv1x1_16_kernel<DT, WM, WN, FM, FN, BK>, a, 32 * FM * WM, 32 * FN * WN, 64 * WM * WN);
}

// the only place that maps a plan to template parameters
template <int DT>
static int launch_plan16(const Conv1x1Args16& a, int config) {
  Conv1x1Plan16 p;
  if (plan_for16(a.M, a.K, config, &p) != MTR_OK) return MTR_E_PARAM;
  if (p.cfg == kCfg16DeepK)
    return a.gate ? launch_conv1x1_16(conv1x1_16_deepk_kernel<DT, true>, a, kDk16BM, kDk16BN, 256)
                  : launch_conv1x1_16(conv1x1_16_deepk_kernel<DT, false>, a, kDk16BM, kDk16BN, 256);
  if (p.cfg == kCfg16Square) return launch_tiles16<DT, 2, 2, 2, 2, 32>(a);
  switch (p.waves_m) {
    case 1: return launch_tiles16<DT, 1, 1, 1, 1, 64>(a);
    case 2: return launch_tiles16<DT, 2, 1, 1, 1, 64>(a);
    case 3: return launch_tiles16<DT, 3, 1, 1, 1, 64>(a);
    case 4: return launch_tiles16<DT, 4, 1, 1, 1, 64>(a);
    default: return launch_tiles16<DT, 5, 1, 1, 1, 64>(a);
  }
}

}  // namespace mtr

extern "C" int mtr_conv1x1_plan16(int M, int K, int HW, long long B, int config, int* plan) {
  if (!plan) return MTR_E_NULL;
  if (B < 0 || M <= 0 || K <= 0 || HW <= 0) return MTR_E_SHAPE;
  mtr::Conv1x1Plan16 p;
  const int e = mtr::plan_for16(M, K, config, &p);
  if (e != MTR_OK) return e;
  plan[0] = p.cfg;
  plan[1] = p.waves_m;
  plan[2] = p.cfg == mtr::kCfg16Square ? 128 : 32 * p.waves_m;
  plan[3] = p.cfg == mtr::kCfg16Square ? 128 : p.cfg == mtr::kCfg16DeepK ? mtr::kDk16BN : 32;
  return MTR_OK;
}

extern "C" int mtr_conv1x1_bias_act16(const void* x, int dtype, const void* weight, const float* bias,
                                      const float* gate, const void* residual, int act, long long B, int M, int K,
                                      int HW, void* y, mtr_stream_t stream) {
  return mtr_conv1x1_bias_act16_opts(x, dtype, weight, bias, gate, residual, act, B, M, K, HW, y, stream, -1);
}

extern "C" int mtr_conv1x1_bias_act16_opts(const void* x, int dtype, const void* weight, const float* bias,
                                           const float* gate, const void* residual, int act, long long B, int M,
                                           int K, int HW, void* y, mtr_stream_t stream, int config) {
  if (!x || !weight || !bias || !y) return MTR_E_NULL;
  if (dtype != MTR_F16 && dtype != MTR_BF16) return MTR_E_DTYPE;
  // 16-byte groups: eight positions of a k-row of x, eight k of a weight row
  if (mtr::conv1x1_shape_check(B, M, K, HW, 8) != MTR_OK) return MTR_E_SHAPE;
  if (act < mtr::kActNone || act > mtr::kActHardswish) return MTR_E_PARAM;
  if (config < -1 || config > mtr::kCfg16DeepK) return MTR_E_PARAM;
  if (((uintptr_t)x % 16) || ((uintptr_t)weight % 16) || ((uintptr_t)y % 16) || ((uintptr_t)residual % 16) ||
      ((uintptr_t)bias % 4) || ((uintptr_t)gate % 4))
    return MTR_E_ALIGN;
  if (x == y || (residual && residual == x)) return MTR_E_PARAM;  // y is written while x is still read
  if (B == 0) return MTR_OK;
  const mtr::Conv1x1Args16 a = {(const unsigned short*)x, (const unsigned short*)weight, bias, gate,
                                 (const unsigned short*)residual, (unsigned short*)y, act, M, K, HW, B * HW,
                                 (hipStream_t)stream};
  return dtype == MTR_F16 ? mtr::launch_plan16<MTR_F16>(a, config) : mtr::launch_plan16<MTR_BF16>(a, config);
}
