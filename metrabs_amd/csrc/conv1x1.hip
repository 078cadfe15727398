// K13: a 1x1 stride-1 NCHW convolution as one f32 MFMA GEMM with the K10 epilogue folded in.
//
// Not part of the reference's hot path (like K10 / K11 / K12): the expand and project convolutions of
// the MBConv blocks of the backbone's inference copy (backbones.fold_batchnorm(fused_epilogue=True)).
// PyTorch-ROCm runs each as a rocBLAS GEMM followed by K10 ("+ bias", activation, "+ skip"), and the
// project conv additionally behind PyTorch's "x * gate" of the squeeze-excite block: two or three
// HBM round trips over an activation beside the GEMM.  Here, per image b:
//
//   y[b, m, p] = act(bias[m] + sum_k W[m, k] * (x[b, k, p] * gate[b, k])) (+ residual[b, m, p])
//
// in one launch.  The GEMM is computed transposed, Y_b^T = X_b^T W^T, on v_mfma_f32_32x32x2_f32 (exact
// f32: a k-ordered fmaf chain per output): the A operand is a 32 (positions) x 2 (k) slice of X, the
// B operand a 2 (k) x 32 (channels) slice of W^T, so every lane ends with four CONSECUTIVE positions
// of one output channel in four accumulator registers -- one 16-byte store per group, the epilogue
// (bias, activation, skip) applied in registers on the way out.
//
// The column index runs over (image, position) jointly: a tile may span images (8x8 maps: 64
// positions per image), each group of four columns carries its own image index (HW % 4 == 0, so a
// group never straddles two images).  Workgroup tile BM x BN, k-tiles of BK staged global -> registers
// -> LDS with two LDS buffers (the next tile's loads are in flight while the current one is
// multiplied).  W is stored transposed in LDS ([k][m]), X as it is ([k][p]); rows past M, columns
// past B * HW and k past K are zero-filled, never stored.  The configuration is a pure function of
// (M, K, HW, B) (pick_config); the k order is 0, 1, 2, ... in every configuration, so the result does
// not depend on it.  No atomics, no split-K: the same inputs give the same bits.
//
// The input prologue (template parameter PRE: -1 none, else an Act code): behind a dense 3x3 convolution
// whose K10 pass ("+ bias", activation, in place) has been left out, every staged element of x becomes
//   v = act_in(x[b, k, p] + in_bias[k])
// made opaque with settled() -- the f32 value K10 would have stored -- and then v * gate[b, k] as above.
// It is applied inside the bounds checks (or selected against zero, deep-K): a zero-filled entry stays zero.
// PRE = -1 is the code from before the prologue existed.
#include <type_traits>

#include "common.h"

namespace mtr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kC1PadX = 32;  // X tile row pad (floats): the two lane halves read rows k, k + 1
constexpr int kC1PadW = 4;   // W^T tile row pad: the transposing writes of 4 k-rows land on distinct banks

// WM x WN waves, each FM x FN tiles of 32 x 32 (channels x positions), k-tiles of BK
template <int WM, int WN, int FM, int FN, int BK, int ACT, int PRE>
__global__ __launch_bounds__(64 * WM * WN) void conv1x1_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ in_bias, const float* __restrict__ gate, const float* __restrict__ residual,
    float* __restrict__ y, int M, int K, int HW, int n_total, FastDiv by_hw) {
  constexpr int NT = 64 * WM * WN;
  constexpr int BM = 32 * FM * WM, BN = 32 * FN * WN;
  constexpr int LDX = BN + kC1PadX, LDW = BM + kC1PadW;
  constexpr int XROW4 = BN / 4;                         // float4 groups per X tile row
  constexpr int XPASS = NT / XROW4;                     // X rows per loader pass
  constexpr int XV = (BK + XPASS - 1) / XPASS;          // loader passes over the X tile
  constexpr int WPASS = NT / (BK / 4);                  // W rows per loader pass
  constexpr int WV = (BM + WPASS - 1) / WPASS;
  static_assert(NT % XROW4 == 0 && NT % (BK / 4) == 0, "loader mapping");
  __shared__ float xs[2][BK * LDX];
  __shared__ float ws[2][BK * LDW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const long long khw = (long long)K * HW;

  // this thread's X column group: fixed for the whole k loop
  const int xn4 = tid % XROW4, xk0 = tid / XROW4;
  const int xcol = n0 + xn4 * 4;
  const bool xcol_ok = xcol < n_total;
  const unsigned xb = xcol_ok ? fastdiv((unsigned)xcol, by_hw) : 0u;
  const float* xsrc = x + (long long)xb * khw + (xcol - (int)xb * HW);
  const float* gsrc = gate ? gate + (long long)xb * K : nullptr;
  // this thread's W rows: k4 fixed, rows strided by WPASS
  const int wk4 = tid % (BK / 4), wr0 = tid / (BK / 4);

  float4 xr[XV], wr[WV];
  auto load_tile = [&](int k0) {
#pragma unroll
    for (int v = 0; v < XV; ++v) {
      const int k = k0 + xk0 + v * XPASS;
      float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (xcol_ok && k < K && xk0 + v * XPASS < BK) {
        t = *reinterpret_cast<const float4*>(xsrc + (long long)k * HW);
        if constexpr (PRE >= 0) {  // the epilogue of the convolution in front: K10's expression, K10's bits
          const float bi = in_bias[k];
          t.x = input_prologue<PRE>(t.x, bi); t.y = input_prologue<PRE>(t.y, bi);
          t.z = input_prologue<PRE>(t.z, bi); t.w = input_prologue<PRE>(t.w, bi);
        }
        if (gsrc) {  // the squeeze-excite gate, once per staged element: x * g rounded as torch does
          const float g = gsrc[k];
          t.x *= g; t.y *= g; t.z *= g; t.w *= g;
        }
      }
      xr[v] = t;
    }
#pragma unroll
    for (int v = 0; v < WV; ++v) {
      const int m = m0 + wr0 + v * WPASS, k = k0 + wk4 * 4;
      float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (m < M && k < K && wr0 + v * WPASS < BM) t = *reinterpret_cast<const float4*>(w + (long long)m * K + k);
      wr[v] = t;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int v = 0; v < XV; ++v) {
      const int r = xk0 + v * XPASS;
      if (r < BK) *reinterpret_cast<float4*>(&xs[buf][r * LDX + xn4 * 4]) = xr[v];
    }
#pragma unroll
    for (int v = 0; v < WV; ++v) {
      const int r = wr0 + v * WPASS;
      if (r < BM) {
        float* d = &ws[buf][(wk4 * 4) * LDW + r];
        d[0] = wr[v].x; d[LDW] = wr[v].y; d[2 * LDW] = wr[v].z; d[3 * LDW] = wr[v].w;
      }
    }
  };

  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

  const int half = lane >> 5, l32 = lane & 31;
  const int n_tiles = (K + BK - 1) / BK;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int t = 0; t < n_tiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < n_tiles) load_tile((t + 1) * BK);  // in flight during this tile's MFMAs
    const float* xb_ = &xs[buf][half * LDX + wn * (32 * FN) + l32];
    const float* wb_ = &ws[buf][half * LDW + wm * (32 * FM) + l32];
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float a[FN], b[FM];
#pragma unroll
      for (int j = 0; j < FN; ++j) a[j] = xb_[kk * LDX + j * 32];
#pragma unroll
      for (int i = 0; i < FM; ++i) b[i] = wb_[kk * LDW + i * 32];
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[i], acc[i][j], 0, 0, 0);
    }
    if (t + 1 < n_tiles) store_tile(buf ^ 1);  // the other buffer: last read before the previous barrier
    __syncthreads();
  }

  // epilogue: lane holds channel m = .. + l32, positions 8 g + 4 half + 0..3 of each 32-column tile
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + wm * (32 * FM) + i * 32 + l32;
    if (m >= M) continue;
    const float bm = bias[m];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = n0 + wn * (32 * FN) + j * 32 + 8 * g + 4 * half;
        if (col >= n_total) continue;
        const unsigned b = fastdiv((unsigned)col, by_hw);
        const long long off = ((long long)b * M + m) * HW + (col - (int)b * HW);
        epilogue_store4<ACT>(acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3], bm,
                             residual, y, off);
      }
    }
  }
}

// The deep-K configuration: few output channels behind a long k loop (the project convolutions of the
// last stages: 8x8 maps, K = 960 .. 1536).  The tall tiles above run those with ONE wave per SIMD, one
// k-tile of global loads in flight and a wait + LDS write + barrier behind every tile's MFMAs that no
// other wave covers.  Here a workgroup of WAVES waves takes 32 WAVES channels (all of M = 256 with 8
// waves: x is read once) x 16 columns on v_mfma_f32_16x16x4_f32 (the same k-ordered fmaf chain per
// output as the 32x32x2 form, so the same bits), which gives twice the waves of a 32-column tile: two
// per SIMD, one's staging under the other's MFMAs.  k-tiles of 32 go global -> registers -> a ring of
// three LDS stages: tile t + 3 is requested before tile t is multiplied and tile t + 2 (requested one
// whole tile earlier) is written to LDS between the two halves of tile t's MFMAs, so a load has two
// tiles of MFMA time to arrive and the barrier follows MFMAs, not LDS writes.  W is staged as it lies in
// memory ([m][k], 16-byte LDS writes, rows 36 floats apart: the fragment reads of 16 rows x 4 k hit
// distinct banks), x as [k][16].
constexpr int kDkBK = 32, kDkBN = 16, kDkStages = 3;
constexpr int kDkLDW = kDkBK + 4;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr size_t deepk_lds_bytes(int waves) {
  return (size_t)kDkStages * (kDkBK * kDkBN + 32 * waves * kDkLDW) * sizeof(float);
}

template <int WAVES, int ACT, int PRE>
__global__ __launch_bounds__(64 * WAVES) void conv1x1_deepk_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ in_bias, const float* __restrict__ gate, const float* __restrict__ residual,
    float* __restrict__ y, int M, int K, int HW, int n_total, FastDiv by_hw) {
  constexpr int NT = 64 * WAVES, BM = 32 * WAVES;
  constexpr int XS = kDkBK * kDkBN, WS = BM * kDkLDW;  // floats per stage
  static_assert(BM * (kDkBK / 4) == 4 * NT, "W loader mapping");
  extern __shared__ float4 dk_lds[];
  float* xs = reinterpret_cast<float*>(dk_lds);  // [stage][k][16]
  float* ws = xs + kDkStages * XS;               // [stage][m][kDkLDW]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * kDkBN;
  const long long khw = (long long)K * HW;

  // x: every thread one k row and XV consecutive columns of the 32 x 16 tile, fixed for the whole k loop
  constexpr int XV = XS / NT;  // 1 (8 waves) or 2 (4 waves)
  static_assert(XV * NT == XS && (XV == 1 || XV == 2), "x loader mapping");
  const int xp = (tid % (kDkBN / XV)) * XV, xk = tid / (kDkBN / XV);
  const int xcol = n0 + xp;
  const bool xcol_ok = xcol < n_total;
  const unsigned xb = xcol_ok ? fastdiv((unsigned)xcol, by_hw) : 0u;
  const float* xsrc = xcol_ok ? x + (long long)xb * khw + (xcol - (int)xb * HW) : x;
  const bool has_gate = gate != nullptr;
  const float* gsrc = has_gate ? gate + (long long)xb * K : x;  // (no gate: any K readable floats, multiplied by 1)
  // W: every thread four 16-byte groups, rows NT / 8 apart
  const int wk4 = tid & 7, wr0 = tid >> 3;

  // Loads carry no condition and no arithmetic, and every thread issues the same ones: a group past M, K or
  // B * HW is read from a clamped address and zeroed (and x multiplied by its gate) on its way to LDS, two
  // tiles later.  A select or a product beside the load makes the loop wait for it at once; a branch around
  // it makes the compiler wait for the loads of the tile before at the next load.
  // Two register sets (tiles t + 2 and t + 3 are in flight together), always indexed by a constant.
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 rw[2][4] = {{zero, zero, zero, zero}, {zero, zero, zero, zero}};
  float rx[2][XV] = {}, rg[2] = {1.0f, 1.0f}, rbi[2] = {0.0f, 0.0f};
  auto load_tile = [&](int kt, auto set) {
    constexpr int P = decltype(set)::value;
    const int k0 = kt * kDkBK;
    const int kx = min(k0 + xk, K - 1);
    if constexpr (XV == 2) {
      const float2 t = *reinterpret_cast<const float2*>(xsrc + (long long)kx * HW);
      rx[P][0] = t.x; rx[P][XV - 1] = t.y;
    } else {
      rx[P][0] = xsrc[(long long)kx * HW];
    }
    rg[P] = gsrc[kx];
    if constexpr (PRE >= 0) rbi[P] = in_bias[kx];
    const int k = min(k0 + wk4 * 4, K - 4);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = min(m0 + wr0 + v * (NT / 8), M - 1);
      rw[P][v] = *reinterpret_cast<const float4*>(w + (long long)m * K + k);
    }
  };
  auto store_tile = [&](int stage, int kt, auto set) {
    constexpr int P = decltype(set)::value;
    const int k0 = kt * kDkBK;
    const float g = has_gate ? rg[P] : 1.0f;  // the squeeze-excite gate, once per staged element: x * g rounded as torch does
    const bool x_ok = xcol_ok && k0 + xk < K;
    float* xd = &xs[stage * XS + xk * kDkBN + xp];
    float v0 = rx[P][0], v1 = rx[P][XV - 1];
    if constexpr (PRE >= 0) {  // the epilogue of the convolution in front: K10's expression, K10's bits.  A clamped
      // load may give anything here (inf, NaN): it is selected away below, never multiplied to zero
      v0 = input_prologue<PRE>(v0, rbi[P]);
      if constexpr (XV == 2) v1 = input_prologue<PRE>(v1, rbi[P]);
    }
    if constexpr (XV == 2) {
      *reinterpret_cast<float2*>(xd) = make_float2(x_ok ? v0 * g : 0.0f, x_ok ? v1 * g : 0.0f);
    } else {
      *xd = x_ok ? v0 * g : 0.0f;
    }
    const bool k_ok = k0 + wk4 * 4 < K;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = wr0 + v * (NT / 8);
      const bool ok = k_ok && m0 + row < M;  // (selects of scalars: a select of two float4 objects goes through memory)
      float4 u = rw[P][v];
      u.x = ok ? u.x : 0.0f; u.y = ok ? u.y : 0.0f; u.z = ok ? u.z : 0.0f; u.w = ok ? u.w : 0.0f;
      *reinterpret_cast<float4*>(&ws[stage * WS + row * kDkLDW + wk4 * 4]) = u;
    }
  };

  f32x4 acc[2];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[f][r] = 0.0f;

  // lane = (column or channel c of the 16, k group kg of the 4)
  const int c = lane & 15, kg = lane >> 4;
  auto multiply = [&](int stage, int kk0) {
    const float* xb_ = &xs[stage * XS + kg * kDkBN + c];
    const float* wb_ = &ws[stage * WS + (wave * 32 + c) * kDkLDW + kg];
#pragma unroll
    for (int kk = kk0; kk < kk0 + kDkBK / 2; kk += 4) {
      const float a = xb_[kk * kDkBN];
      const float b0 = wb_[kk], b1 = wb_[16 * kDkLDW + kk];
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[1], 0, 0, 0);
    }
  };

  const int n_tiles = (K + kDkBK - 1) / kDkBK;
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
    if (!G || t + 3 < n_tiles) load_tile(t + 3, issue);
    multiply(stage, 0);
    __builtin_amdgcn_sched_barrier(0);
    // stage of tile t + 2 = stage of tile t - 1: last read before the previous barrier
    if (!G || t + 2 < n_tiles) store_tile(stage == 0 ? 2 : stage - 1, t + 2, hold);
    __builtin_amdgcn_sched_barrier(0);
    multiply(stage, kDkBK / 2);
    stage = stage == 2 ? 0 : stage + 1;
    __syncthreads();
  };
  // the body of the loop has no condition (see load_tile); the last steps, which have, run apart
  int t = 0;
  for (; t + 4 < n_tiles; t += 2) {
    step(t, ra, rb, std::false_type{});
    step(t + 1, rb, ra, std::false_type{});
  }
  for (; t < n_tiles; t += 2) {
    step(t, ra, rb, std::true_type{});
    if (t + 1 < n_tiles) step(t + 1, rb, ra, std::true_type{});
  }

  // epilogue: lane holds channel .. + c, positions 4 kg + 0..3 of the 16 columns
  const int col = n0 + 4 * kg;
  if (col >= n_total) return;
  const unsigned b = fastdiv((unsigned)col, by_hw);
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int m = m0 + wave * 32 + f * 16 + c;
    if (m >= M) continue;
    const float bm = bias[m];
    const long long off = ((long long)b * M + m) * HW + (col - (int)b * HW);
    epilogue_store4<ACT>(acc[f][0], acc[f][1], acc[f][2], acc[f][3], bm, residual, y, off);
  }
}

// The 64 x 64 ring-staged configuration ('deep64'): the deep-K pipeline above on a tile that re-reads half as much.
// deep-K's 256 x 16 tile reads the whole of W once per 16 columns (1536 -> 256 on 8x8 maps at batch 64: 400 MB of W
// from L2 per layer); here a workgroup of eight waves takes 64 channels x 64 columns, every wave 32 channels x 16
// columns on v_mfma_f32_16x16x4_f32 (two independent accumulators: the MFMA issues every 32 cycles, a dependent one
// after 40), two waves per SIMD on a CU that holds one workgroup.  k-tiles of 32 go global -> registers -> a ring of
// three LDS stages exactly as above: tile t + 3 is requested before tile t is multiplied, tile t + 2 is written to
// LDS between the halves of tile t's MFMAs, one barrier per tile behind MFMAs.  Every thread stages ONE 16-byte group
// of x and ONE of W per tile.  W lies in LDS as in memory ([m][k], rows 34 floats apart, two 8-byte writes per
// group: the fragment reads of 16 rows x 2 k per half-wave hit 32 distinct banks), x as [k][64] with the 16-column
// groups of odd k rows swapped in pairs (the fragment reads of 2 k x 16 columns per half-wave hit 32 distinct banks
// without a pad).  16.5 KB per stage, 49.5 KB in all: three workgroups per CU on the larger maps.
// The loads carry no condition and no arithmetic: pointers walked by one tile over the whole tiles, clamped addresses
// in the last steps; the zero-fill, the prologue and the gate product are applied on the way to LDS (a zero-filled
// entry is selected, so it stays zero).  Each lane ends with four consecutive positions of one channel, a wave's
// store instruction writes 64-byte row segments.  The k order is 0, 1, 2, ... as everywhere: the same bits.
constexpr int kD6BM = 64, kD6BN = 64, kD6BK = 32, kD6Stages = 3, kD6Waves = 8;
constexpr int kD6LDW = kD6BK + 2;

template <int ACT, int PRE>
__global__ __launch_bounds__(64 * kD6Waves) void conv1x1_deep64_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ in_bias, const float* __restrict__ gate, const float* __restrict__ residual,
    float* __restrict__ y, int M, int K, int HW, int n_total, FastDiv by_hw) {
  constexpr int NT = 64 * kD6Waves, BM = kD6BM, BN = kD6BN, BK = kD6BK, LDW = kD6LDW;
  constexpr int XS = BK * BN, WS = BM * LDW;  // floats per stage
  static_assert(BK * (BN / 4) == NT && BM * (BK / 4) == NT, "loader mappings: one 16-byte group of x and of W each");
  __shared__ __attribute__((aligned(16))) float d6_lds[kD6Stages * (XS + WS)];
  float* xs = d6_lds;                   // [stage][k][64], columns ^ 16 in odd rows
  float* ws = d6_lds + kD6Stages * XS;  // [stage][m][LDW]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const long long khw = (long long)K * HW;

  // x: every thread one k row and four consecutive columns of the 32 x 64 tile, fixed for the whole k loop
  const int xn4 = tid & 15, xk = tid >> 4;
  const int xcol = n0 + 4 * xn4;
  const bool xcol_ok = xcol < n_total;
  const unsigned xb = xcol_ok ? fastdiv((unsigned)xcol, by_hw) : 0u;
  const float* xsrc = xcol_ok ? x + (long long)xb * khw + (xcol - (int)xb * HW) : x;
  const bool has_gate = gate != nullptr;
  const float* gsrc = has_gate ? gate + (long long)xb * K : x;  // (no gate: any K readable floats, multiplied by 1)
  const int xdst = xk * BN + ((4 * xn4) ^ ((xk & 1) << 4));
  // W: every thread one row and four consecutive k of the 64 x 32 tile
  const int wk4 = tid & 7, wr = tid >> 3;
  const float* wsrc = w + (long long)min(m0 + wr, M - 1) * K;
  const bool wrow_ok = m0 + wr < M;
  const int wdst = wr * LDW + 4 * wk4;
  // the main loop's loads (whole tiles: nothing to clamp) walk pointers, tile 3 first
  const float* xcur = xsrc + (long long)(3 * BK + xk) * HW;
  const float* gcur = gsrc + 3 * BK + xk;
  const float* bcur = PRE >= 0 ? in_bias + 3 * BK + xk : nullptr;
  const float* wcur = wsrc + 3 * BK + 4 * wk4;
  const long long xadv = (long long)BK * HW;

  // Two register sets (tiles t + 2 and t + 3 are in flight together), always indexed by a constant.
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float4 rx[2] = {zero, zero}, rw[2] = {zero, zero};
  float rg[2] = {1.0f, 1.0f}, rbi[2] = {0.0f, 0.0f};
  auto load_tile = [&](int kt, auto set) {
    constexpr int P = decltype(set)::value;
    const int k0 = kt * BK;
    const int kx = min(k0 + xk, K - 1);
    rx[P] = *reinterpret_cast<const float4*>(xsrc + (long long)kx * HW);
    rg[P] = gsrc[kx];
    if constexpr (PRE >= 0) rbi[P] = in_bias[kx];
    rw[P] = *reinterpret_cast<const float4*>(wsrc + min(k0 + 4 * wk4, K - 4));
  };
  auto load_next_whole_tile = [&](auto set) {
    constexpr int P = decltype(set)::value;
    rx[P] = *reinterpret_cast<const float4*>(xcur);
    rg[P] = *gcur;
    if constexpr (PRE >= 0) rbi[P] = *bcur;
    rw[P] = *reinterpret_cast<const float4*>(wcur);
    xcur += xadv; gcur += BK; wcur += BK;
    if constexpr (PRE >= 0) bcur += BK;
  };
  auto store_tile = [&](int stage, int kt, auto set) {
    constexpr int P = decltype(set)::value;
    const int k0 = kt * BK;
    const float g = has_gate ? rg[P] : 1.0f;  // the squeeze-excite gate, once per staged element: x * g rounded as torch does
    const bool x_ok = xcol_ok && k0 + xk < K;
    float4 v = rx[P];
    if constexpr (PRE >= 0) {  // the epilogue of the convolution in front: K10's expression, K10's bits.  A clamped
      // load may give anything here (inf, NaN): it is selected away below, never multiplied to zero
      const float bi = rbi[P];
      v.x = input_prologue<PRE>(v.x, bi); v.y = input_prologue<PRE>(v.y, bi);
      v.z = input_prologue<PRE>(v.z, bi); v.w = input_prologue<PRE>(v.w, bi);
    }
    v.x = x_ok ? v.x * g : 0.0f; v.y = x_ok ? v.y * g : 0.0f; v.z = x_ok ? v.z * g : 0.0f; v.w = x_ok ? v.w * g : 0.0f;
    *reinterpret_cast<float4*>(&xs[stage * XS + xdst]) = v;
    const bool ok = wrow_ok && k0 + 4 * wk4 < K;  // (selects of scalars: a select of two float4 objects goes through memory)
    const float4 u = rw[P];
    float* wd = &ws[stage * WS + wdst];
    *reinterpret_cast<float2*>(wd) = make_float2(ok ? u.x : 0.0f, ok ? u.y : 0.0f);
    *reinterpret_cast<float2*>(wd + 2) = make_float2(ok ? u.z : 0.0f, ok ? u.w : 0.0f);
  };

  f32x4 acc[2];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[f][r] = 0.0f;

  // lane = (column or channel c of the 16, k group kg of the 4)
  const int c = lane & 15, kg = lane >> 4;
  const int xfrag = kg * BN + ((wn * 16 + c) ^ ((kg & 1) << 4));
  const int wfrag = (wm * 32 + c) * LDW + kg;
  auto multiply = [&](int stage, int kk0) {
    const float* xb_ = &xs[stage * XS + xfrag];
    const float* wb_ = &ws[stage * WS + wfrag];
#pragma unroll
    for (int kk = kk0; kk < kk0 + BK / 2; kk += 4) {
      const float a = xb_[kk * BN];
      const float b0 = wb_[kk], b1 = wb_[16 * LDW + kk];
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b1, acc[1], 0, 0, 0);
    }
  };

  const int n_tiles = (K + BK - 1) / BK, n_whole = K / BK;
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
    multiply(stage, BK / 2);
    stage = stage == 2 ? 0 : stage + 1;
    __syncthreads();
  };
  // the body of the loop has no condition around its loads; the last steps, which have, run apart
  int t = 0;
  for (; t + 4 < n_whole; t += 2) {  // tiles t + 3 and t + 4 are whole
    step(t, ra, rb, std::false_type{});
    step(t + 1, rb, ra, std::false_type{});
  }
  for (; t < n_tiles; t += 2) {
    step(t, ra, rb, std::true_type{});
    if (t + 1 < n_tiles) step(t + 1, rb, ra, std::true_type{});
  }

  // epilogue: lane holds channel .. + c, positions 4 kg + 0..3 of the wave's 16 columns
  const int col = n0 + wn * 16 + 4 * kg;
  if (col >= n_total) return;
  const unsigned b = fastdiv((unsigned)col, by_hw);
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int m = m0 + wm * 32 + f * 16 + c;
    if (m >= M) continue;
    const float bm = bias[m];
    const long long off = ((long long)b * M + m) * HW + (col - (int)b * HW);
    epilogue_store4<ACT>(acc[f][0], acc[f][1], acc[f][2], acc[f][3], bm, residual, y, off);
  }
}

// The streaming configuration: short-K, few-channel projects (the FusedMBConv projects: K <= 256, M <= 64) whose whole
// weight fits LDS.  There every element of x is used by one workgroup only, so its round trip through LDS in the
// tiles above buys no reuse and costs a write, a barrier and a read per k-tile -- and with the input prologue the
// staging threads' VALU work sits in front of that barrier.  Here a workgroup of four waves stages W^T ([k][m], zero
// rows up to a multiple of 32 k, zero columns up to MT * 32) and in_bias into LDS ONCE, behind one barrier, and issues
// no barrier after that.  Each wave owns 32 columns and ALL M rows (MT tiles of 32): lane l loads its A operand of
// v_mfma_f32_32x32x2_f32 straight from global memory, x[k + (l >> 5)][p0 + (l & 31)] (two full 128-byte segments per
// instruction), applies the prologue and the gate to that register and reads the B operand from LDS.  Loads run one
// chunk of kStR k-steps (32 k, 4 KB per wave) ahead of the MFMAs in a second register set; they carry no condition: k
// past K and columns past B * HW read a clamped address and are SELECTED to zero (act(0 + b) is not zero, 0 * inf is
// NaN).  The k order is 0, 1, 2, ... and the accumulator layout that of conv1x1_kernel: the same bits, the same
// epilogue.  A tile may span images (HW < 32): every lane derives its own image index.  `tiles` column tiles per wave,
// one after the other (the weight is staged once for all of them).
constexpr int kStR = 16;                       // k-steps (2 k each) per register chunk
constexpr int kStWaves = 4;
constexpr size_t kStMaxWeight = 64 * 1024;     // bytes of staged W^T: two workgroups per CU (160 KB of LDS)

inline int stream_kpad(int K) { return (K + 2 * kStR - 1) / (2 * kStR) * (2 * kStR); }
inline bool stream_fits(int M, int K) {
  return M <= 96 && (size_t)stream_kpad(K) * ((M + 31) / 32 * 32) * sizeof(float) <= kStMaxWeight;
}

template <int MT, int PRE, bool GATE>
__global__ __launch_bounds__(64 * kStWaves) void conv1x1_stream_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ in_bias, const float* __restrict__ gate, const float* __restrict__ residual,
    float* __restrict__ y, int M, int K, int HW, int n_total, FastDiv by_hw, int act, int tiles) {
  constexpr int NT = 64 * kStWaves, LDW = 32 * MT;
  extern __shared__ float4 st_lds[];
  const int Kpad = (K + 2 * kStR - 1) / (2 * kStR) * (2 * kStR);
  float* ws = reinterpret_cast<float*>(st_lds);  // [Kpad][LDW]: W^T
  float* bs = ws + Kpad * LDW;                   // [Kpad]: in_bias (PRE only)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, l32 = lane & 31;
  const long long khw = (long long)K * HW;
  const int n_chunks = Kpad / (2 * kStR);
  const int n0 = blockIdx.x * (32 * kStWaves * tiles);

  int col0 = 0;            // first column of this wave's current tile
  bool ok = false;         // this lane's column is inside B * HW
  const float* xsrc = x;   // this lane's column, row `half`
  const float* gsrc = x;
  auto enter_tile = [&](int tile) {
    col0 = n0 + tile * 32;
    const int col = col0 + l32;
    ok = col < n_total;
    const unsigned b = ok ? fastdiv((unsigned)col, by_hw) : 0u;
    xsrc = x + (long long)b * khw + (long long)half * HW + (ok ? col - (int)b * HW : 0);
    if constexpr (GATE) gsrc = gate + (long long)b * K + half;
  };

  float xa[kStR], xb[kStR], ga[kStR], gb[kStR];
  auto load_chunk = [&](int c, float (&xr)[kStR], float (&gr)[kStR]) {
#pragma unroll
    for (int j = 0; j < kStR; ++j) {
      const int kk = min(c * (2 * kStR) + 2 * j, K - 2);  // (K % 4 == 0: rows kk, kk + 1 exist)
      xr[j] = xsrc[(long long)kk * HW];
      if constexpr (GATE) gr[j] = gsrc[kk];
    }
  };

  f32x16 acc[MT];
  auto multiply_chunk = [&](int c, const float (&xr)[kStR], const float (&gr)[kStR]) {
#pragma unroll
    for (int j = 0; j < kStR; ++j) {
      const int k = c * (2 * kStR) + 2 * j;
      float v = xr[j];
      // the epilogue of the convolution in front: K10's expression, K10's bits
      if constexpr (PRE >= 0) v = input_prologue<PRE>(v, bs[k + half]);
      if constexpr (GATE) v *= gr[j];  // the squeeze-excite gate: x * g rounded as torch does
      v = (ok && k < K) ? v : 0.0f;
      const float* wb_ = &ws[(k + half) * LDW + l32];
#pragma unroll
      for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(v, wb_[i * 32], acc[i], 0, 0, 0);
    }
  };

  enter_tile(wave);
  load_chunk(0, xa, ga);  // in flight while the weight is staged

  // W^T: consecutive lanes take consecutive channels (conflict-free LDS writes), four k each
  for (int e = tid; e < (Kpad / 4) * LDW; e += NT) {
    const int m = e % LDW, k = (e / LDW) * 4;
    float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (m < M && k < K) t = *reinterpret_cast<const float4*>(w + (long long)m * K + k);
    float* d = &ws[k * LDW + m];
    d[0] = t.x; d[LDW] = t.y; d[2 * LDW] = t.z; d[3 * LDW] = t.w;
  }
  if constexpr (PRE >= 0)
    for (int k = tid; k < Kpad; k += NT) bs[k] = k < K ? in_bias[k] : 0.0f;
  __syncthreads();

  for (int tile = wave;;) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    int c = 0;
    for (; c + 1 < n_chunks; c += 2) {
      load_chunk(c + 1, xb, gb);
      multiply_chunk(c, xa, ga);
      load_chunk(c + 2, xa, ga);  // (past the last chunk: the clamped rows again, not used)
      multiply_chunk(c + 1, xb, gb);
    }
    if (c < n_chunks) multiply_chunk(c, xa, ga);

    // epilogue: lane holds channel m = .. + l32, positions 8 g + 4 half + 0..3 of the tile
    auto epilogue = [&](auto tag) {
      constexpr int ACT = decltype(tag)::value;
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int m = i * 32 + l32;
        if (m >= M) continue;
        const float bm = bias[m];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int col = col0 + 8 * g + 4 * half;
          if (col >= n_total) continue;
          const unsigned b = fastdiv((unsigned)col, by_hw);
          const long long off = ((long long)b * M + m) * HW + (col - (int)b * HW);
          epilogue_store4<ACT>(acc[i][4 * g + 0], acc[i][4 * g + 1], acc[i][4 * g + 2], acc[i][4 * g + 3], bm, residual,
                               y, off);
        }
      }
    };
    with_act(act, epilogue);

    tile += kStWaves;
    if (tile >= kStWaves * tiles) break;
    enter_tile(tile);
    load_chunk(0, xa, ga);
  }
}

// The tile table.  Chosen from the shape only; see DESIGN.md section 11 for the measurements.
//   wide  (WM 2, WN 2, FM 3, FN 2): 192 x 128 -- many output channels (expand), when it still gives
//                                    >= 512 workgroups
//   square(WM 2, WN 2, FM 2, FN 2): 128 x 128 -- the other expand shapes
//   tall  (WM w, WN 1, FM 1, FN 1): 32 w x 32, w = ceil(M / 32) <= 5 -- few output channels (project):
//                                    the whole of M in one workgroup, every position read once.  BK 32
//                                    at w = 4 (one wave per SIMD: half the barriers per MFMA), BK 16
//                                    elsewhere (at w = 5 the BK-32 tiles take 58 KB of LDS, one
//                                    workgroup per CU, 25 % slower)
//   deepk (WAVES w, 32 w x 16, k-tiles of 32 in a ring of three): few output channels behind a long k
//                                    loop (conv1x1_deepk_kernel above), w = 4 or 8
//   stream(4 waves, each 32 t x 32 columns and all of M <= 96): the whole weight in LDS, x straight from global
//                                    memory into the MFMA operand (conv1x1_stream_kernel above); a shape whose
//                                    weight does not fit resolves to tall
//   deep64(8 waves, each 32 x 16 of a 64 x 64 tile, k-tiles of 32 in a ring of three): deep-K's pipeline with half
//                                    its W traffic (conv1x1_deep64_kernel above); takes every shape
enum Conv1x1Config {
  kCfgWide = 0, kCfgSquare = 1, kCfgTall = 2, kCfgDeepK = 3, kCfgStream = 4, kCfgDeep64 = 5, kCfgCount = 6
};

struct Conv1x1Plan { int cfg, waves_m, bm, bn; };

inline Conv1x1Plan plan_tall(int M) {
  const int w = M <= 160 ? (M + 31) / 32 : 4;  // more than 160 channels: rows of 128-channel workgroups
  return {kCfgTall, w, 32 * w, 32};
}
inline Conv1x1Plan plan_deepk(int M) {
  const int w = M <= 128 ? 4 : 8;
  return {kCfgDeepK, w, 32 * w, kDkBN};
}

inline Conv1x1Plan plan_deep64() { return {kCfgDeep64, 2, kD6BM, kD6BN}; }  // waves_m: 2 x 4 waves

// waves_m: the 32-row tiles every wave holds; bn: 128 columns per pass, two passes per workgroup where that still
// leaves 1024 workgroups (one round of four per CU), so the weight is staged half as often
inline Conv1x1Plan plan_stream(int M, int K, int HW, long long B) {
  if (!stream_fits(M, K)) return plan_tall(M);
  const int t = (B * HW + 127) / 128 >= 2048 ? 2 : 1;
  return {kCfgStream, (M + 31) / 32, (M + 31) / 32 * 32, 32 * kStWaves * t};
}

// The classes that measured faster on the 64 x 64 ring-staged tiles than on what they ran before, in every one of five
// alternated rounds of graph replays at batch 64 (EfficientNetV2-S at 256 px): (M, K, HW).  A
// list, not a rule: the same tiles lose where M is far from a multiple of 64 or K is short (MobileNetV3's M = 24, 80,
// 200, 240, its expands behind K <= 112), and an unmeasured shape keeps the kernel it had.  (The four FusedMBConv
// project classes measured faster too and are not here: see that section.)
inline bool deep64_measured_faster(int M, int K, int HW) {
  static const int classes[][3] = {
      {256, 64, 1024}, {128, 256, 256}, {512, 128, 256}, {128, 512, 256},  // stage 4
      {160, 768, 256}, {960, 160, 256}, {160, 960, 256},                   // stage 5
      {256, 960, 64},  {1536, 256, 64}, {256, 1536, 64}, {1280, 256, 64},  // stage 6 and the head
  };
  for (const auto& c : classes)
    if (c[0] == M && c[1] == K && c[2] == HW) return true;
  return false;
}

inline Conv1x1Plan pick_config(int M, int K, int HW, long long B) {
  const long long n_total = B * HW;
  const long long n_tiles128 = (n_total + 127) / 128;
  if (deep64_measured_faster(M, K, HW)) return plan_deep64();
  // the FusedMBConv projects on 64x64 maps (96 -> 48: 44.2 us against 52.9 on the tall tiles with the SiLU prologue,
  // 192 -> 48: 116.0 against 119.4, batch 64, every round); 192 -> 64 and 256 -> 64 on 32x32 maps measured 3 - 5 %
  // slower streamed and stay tall
  if (M == 48 && K <= 192 && HW == 4096 && stream_fits(M, K)) return plan_stream(M, K, HW, B);
  if (M <= 160) return plan_tall(M);
  // project at 8x8: deep-K (960 -> 256: 30.4 us against 35.3, 1536 -> 256: 48.6 against 61.6 at batch 64); larger
  // maps keep two workgroups per 32 columns
  if (M == 256 && K >= 512) return HW <= 64 ? plan_deepk(M) : plan_tall(M);
  // many output channels over a short k loop and few columns (256 -> 1536 and the 256 -> 1280 head at 8x8, batch
  // 64): 128 x 128 tiles give 1.5 rounds of workgroups on 256 CUs, 128 x 32 tiles twelve even ones (40.4 us against
  // 48.0, 38.9 against 47.0)
  if (M >= 1024 && M % 128 == 0 && K <= 256 && n_tiles128 <= 32) return plan_tall(M);
  if (M % 192 == 0 && (M / 192) * n_tiles128 >= 512) return {kCfgWide, 2, 192, 128};
  return {kCfgSquare, 2, 128, 128};
}

// config: -1 the library's own choice, else a Conv1x1Config forced on the shape (every one takes every shape; stream
// where the weight does not fit LDS as tall)
inline int plan_for(int M, int K, int HW, long long B, int config, Conv1x1Plan* p) {
  switch (config) {
    case -1: *p = pick_config(M, K, HW, B); return MTR_OK;
    case kCfgWide: *p = {kCfgWide, 2, 192, 128}; return MTR_OK;
    case kCfgSquare: *p = {kCfgSquare, 2, 128, 128}; return MTR_OK;
    case kCfgTall: *p = plan_tall(M); return MTR_OK;
    case kCfgDeepK: *p = plan_deepk(M); return MTR_OK;
    case kCfgStream: *p = plan_stream(M, K, HW, B); return MTR_OK;
    case kCfgDeep64: *p = plan_deep64(); return MTR_OK;
    default: return MTR_E_PARAM;
  }
}

// One K13 launch's arguments, as the entry point has checked them
struct Conv1x1Args {
  const float *x, *w, *bias, *in_bias, *gate, *residual;
  float* y;
  int act, in_act, M, K, HW;
  long long n_total;
  hipStream_t stream;
};

// Launches `kern` on a grid of bm-channel x bn-column tiles; `extra`: the kernel's arguments behind by_hw (stream's)
template <typename Kern, typename... Extra>
static int launch_conv1x1(Kern kern, const Conv1x1Args& a, int bm, int bn, int threads, size_t lds, Extra... extra) {
  const long long gx = (a.n_total + bn - 1) / bn, gy = (a.M + bm - 1) / bm;
  if (gx > 0x7fffffffLL || gy > 65535) return MTR_E_SHAPE;
  if (lds > 64 * 1024) {
    const int e = allow_dynamic_lds((const void*)kern, lds);
    if (e != MTR_OK) return e;
  }
  MTR_CLEAR_STALE();
  hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(threads), lds, a.stream, a.x, a.w, a.bias, a.in_bias,
                     a.gate, a.residual, a.y, a.M, a.K, a.HW, (int)a.n_total, make_fastdiv((unsigned)a.HW), extra...);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

// f(pre, act): the tags of the kernels' template parameters PRE (-1: no prologue, in_bias is NULL) and ACT
template <typename F>
static int dispatch_pre_act(const Conv1x1Args& a, F&& f) {
  return dispatch_pre(a.in_bias, a.in_act,
                      [&](auto pre) { return dispatch_act(a.act, [&](auto act) { return f(pre, act); }); });
}

template <int WM, int WN, int FM, int FN, int BK>
static int launch_tiles(const Conv1x1Args& a) {
  return dispatch_pre_act(a, [&](auto pre, auto act) {
    return launch_conv1x1(conv1x1_kernel<WM, WN, FM, FN, BK, decltype(act)::value, decltype(pre)::value>, a,
                          32 * FM * WM, 32 * FN * WN, 64 * WM * WN, 0);
  });
}

template <int WAVES>
static int launch_deepk(const Conv1x1Args& a) {
  return dispatch_pre_act(a, [&](auto pre, auto act) {
    return launch_conv1x1(conv1x1_deepk_kernel<WAVES, decltype(act)::value, decltype(pre)::value>, a, 32 * WAVES,
                          kDkBN, 64 * WAVES, deepk_lds_bytes(WAVES));
  });
}

static int launch_deep64(const Conv1x1Args& a) {
  return dispatch_pre_act(a, [&](auto pre, auto act) {
    return launch_conv1x1(conv1x1_deep64_kernel<decltype(act)::value, decltype(pre)::value>, a, kD6BM, kD6BN,
                          64 * kD6Waves, 0);
  });
}

// bn: the plan's columns per workgroup, 128 per pass (one grid row: every wave holds all MT row tiles)
template <int MT>
static int launch_stream(const Conv1x1Args& a, int bn) {
  return dispatch_pre(a.in_bias, a.in_act, [&](auto pre) {
    constexpr int PRE = decltype(pre)::value;
    const int kpad = stream_kpad(a.K), tiles = bn / (32 * kStWaves);
    const size_t lds = ((size_t)kpad * 32 * MT + (PRE >= 0 ? kpad : 0)) * sizeof(float);
    const auto go = [&](auto kern) { return launch_conv1x1(kern, a, 32 * MT, bn, 64 * kStWaves, lds, a.act, tiles); };
    return a.gate ? go(conv1x1_stream_kernel<MT, PRE, true>) : go(conv1x1_stream_kernel<MT, PRE, false>);
  });
}

}  // namespace mtr

extern "C" int mtr_conv1x1_plan(int M, int K, int HW, long long B, int config, int* plan) {
  if (!plan) return MTR_E_NULL;
  if (B < 0 || M <= 0 || K <= 0 || HW <= 0) return MTR_E_SHAPE;
  mtr::Conv1x1Plan p;
  const int e = mtr::plan_for(M, K, HW, B, config, &p);
  if (e != MTR_OK) return e;
  plan[0] = p.cfg; plan[1] = p.waves_m; plan[2] = p.bm; plan[3] = p.bn;
  return MTR_OK;
}

extern "C" int mtr_conv1x1_bias_act(const void* x, int dtype, const float* weight, const float* bias,
                                    const float* gate, const void* residual, int act, long long B, int M,
                                    int K, int HW, void* y, mtr_stream_t stream) {
  return mtr_conv1x1_bias_act_pre(x, dtype, weight, bias, nullptr, mtr::kActNone, gate, residual, act, B, M, K, HW, y,
                                  stream, -1);
}

extern "C" int mtr_conv1x1_bias_act_opts(const void* x, int dtype, const float* weight, const float* bias,
                                         const float* gate, const void* residual, int act, long long B,
                                         int M, int K, int HW, void* y, mtr_stream_t stream, int config) {
  if (config > mtr::kCfgDeepK) return x && weight && bias && y ? MTR_E_PARAM : MTR_E_NULL;  // (stream: the _pre entry)
  return mtr_conv1x1_bias_act_pre(x, dtype, weight, bias, nullptr, mtr::kActNone, gate, residual, act, B, M, K, HW, y,
                                  stream, config);
}

extern "C" int mtr_conv1x1_bias_act_pre(const void* x, int dtype, const float* weight, const float* bias,
                                        const float* in_bias, int in_act, const float* gate, const void* residual,
                                        int act, long long B, int M, int K, int HW, void* y, mtr_stream_t stream,
                                        int config) {
  if (!x || !weight || !bias || !y) return MTR_E_NULL;
  if (dtype != MTR_F32) return MTR_E_DTYPE;
  // 16-byte groups: four positions of x / y / residual, four k of a weight row
  if (mtr::conv1x1_shape_check(B, M, K, HW, 4) != MTR_OK) return MTR_E_SHAPE;
  if (act < mtr::kActNone || act > mtr::kActHardswish) return MTR_E_PARAM;
  if (in_act < mtr::kActNone || in_act > mtr::kActHardswish) return MTR_E_PARAM;
  if (!in_bias && in_act != mtr::kActNone) return MTR_E_PARAM;  // an input activation belongs to an input bias
  if (((uintptr_t)x % 16) || ((uintptr_t)weight % 16) || ((uintptr_t)y % 16) || ((uintptr_t)residual % 16) ||
      ((uintptr_t)in_bias % 4))
    return MTR_E_ALIGN;
  if (x == y || (residual && residual == x)) return MTR_E_PARAM;  // y is written while x is still read
  if (B == 0) return MTR_OK;
  const mtr::Conv1x1Args a = {(const float*)x, weight, bias, in_bias, gate, (const float*)residual, (float*)y,
                               act, in_act, M, K, HW, B * HW, (hipStream_t)stream};
  mtr::Conv1x1Plan p;
  if (mtr::plan_for(M, K, HW, B, config, &p) != MTR_OK) return MTR_E_PARAM;
  switch (p.cfg) {
    case mtr::kCfgWide: return mtr::launch_tiles<2, 2, 3, 2, 16>(a);
    case mtr::kCfgSquare: return mtr::launch_tiles<2, 2, 2, 2, 16>(a);
    case mtr::kCfgStream:
      switch (p.waves_m) {
        case 1: return mtr::launch_stream<1>(a, p.bn);
        case 2: return mtr::launch_stream<2>(a, p.bn);
        default: return mtr::launch_stream<3>(a, p.bn);
      }
    case mtr::kCfgDeep64: return mtr::launch_deep64(a);
    case mtr::kCfgDeepK:
      switch (p.waves_m) {
        case 4: return mtr::launch_deepk<4>(a);
        default: return mtr::launch_deepk<8>(a);
      }
    default:
      switch (p.waves_m) {
        case 1: return mtr::launch_tiles<1, 1, 1, 1, 16>(a);
        case 2: return mtr::launch_tiles<2, 1, 1, 1, 16>(a);
        case 3: return mtr::launch_tiles<3, 1, 1, 1, 16>(a);
        case 4: return mtr::launch_tiles<4, 1, 1, 1, 32>(a);
        default: return mtr::launch_tiles<5, 1, 1, 1, 16>(a);
      }
  }
}
