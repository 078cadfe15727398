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
#include "common.h"

namespace mtr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kC1PadX = 32;  // X tile row pad (floats): the two lane halves read rows k, k + 1
constexpr int kC1PadW = 4;   // W^T tile row pad: the transposing writes of 4 k-rows land on distinct banks

// WM x WN waves, each FM x FN tiles of 32 x 32 (channels x positions), k-tiles of BK
template <int WM, int WN, int FM, int FN, int BK, int ACT>
__global__ __launch_bounds__(64 * WM * WN) void conv1x1_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    const float* __restrict__ gate, const float* __restrict__ residual, float* __restrict__ y, int M,
    int K, int HW, int n_total, FastDiv by_hw) {
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
        float4 r;
        r.x = activate<ACT>(acc[i][j][4 * g + 0] + bm);
        r.y = activate<ACT>(acc[i][j][4 * g + 1] + bm);
        r.z = activate<ACT>(acc[i][j][4 * g + 2] + bm);
        r.w = activate<ACT>(acc[i][j][4 * g + 3] + bm);
        if (residual) {  // the block's skip connection, added after the activation (K10's order)
          const float4 q = *reinterpret_cast<const float4*>(residual + off);
          r.x += q.x; r.y += q.y; r.z += q.z; r.w += q.w;
        }
        *reinterpret_cast<float4*>(y + off) = r;
      }
    }
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
enum Conv1x1Config { kCfgWide = 0, kCfgSquare = 1, kCfgTall = 2 };

struct Conv1x1Plan { int cfg, waves_m, bm, bn; };

inline Conv1x1Plan pick_config(int M, int K, int HW, long long B) {
  const long long n_total = B * HW;
  const long long n_tiles128 = (n_total + 127) / 128;
  if (M <= 160) {
    const int w = (M + 31) / 32;
    return {kCfgTall, w, 32 * w, 32};
  }
  if (M == 256 && K >= 512) return {kCfgTall, 4, 128, 32};  // project at 8x8: two workgroups per 32 columns
  if (M % 192 == 0 && (M / 192) * n_tiles128 >= 512) return {kCfgWide, 2, 192, 128};
  return {kCfgSquare, 2, 128, 128};
}

template <int WM, int WN, int FM, int FN, int BK>
static int launch_conv1x1_cfg(const float* x, const float* w, const float* bias, const float* gate,
                              const float* residual, float* y, int act, int M, int K, int HW,
                              long long n_total, hipStream_t stream) {
  constexpr int BM = 32 * FM * WM, BN = 32 * FN * WN;
  const long long gx = (n_total + BN - 1) / BN, gy = (M + BM - 1) / BM;
  if (gx > 0x7fffffffLL || gy > 65535) return MTR_E_SHAPE;
  const dim3 grid((unsigned)gx, (unsigned)gy), block(64 * WM * WN);
  const FastDiv by_hw = make_fastdiv((unsigned)HW);
  MTR_CLEAR_STALE();
#define MTR_C1_LAUNCH(ACT)                                                                                    \
  hipLaunchKernelGGL((conv1x1_kernel<WM, WN, FM, FN, BK, ACT>), grid, block, 0, stream, x, w, bias, gate, residual, \
                     y, M, K, HW, (int)n_total, by_hw)
  switch (act) {
    case kActNone: MTR_C1_LAUNCH(kActNone); break;
    case kActRelu: MTR_C1_LAUNCH(kActRelu); break;
    case kActSilu: MTR_C1_LAUNCH(kActSilu); break;
    case kActHardswish: MTR_C1_LAUNCH(kActHardswish); break;
    default: return MTR_E_PARAM;
  }
#undef MTR_C1_LAUNCH
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

}  // namespace mtr

extern "C" int mtr_conv1x1_bias_act(const void* x, int dtype, const float* weight, const float* bias,
                                    const float* gate, const void* residual, int act, long long B, int M,
                                    int K, int HW, void* y, mtr_stream_t stream) {
  if (!x || !weight || !bias || !y) return MTR_E_NULL;
  if (dtype != MTR_F32) return MTR_E_DTYPE;
  if (B < 0 || M <= 0 || K <= 0 || HW <= 0) return MTR_E_SHAPE;
  // 16-byte groups: four positions of x / y / residual, four k of a weight row
  if (HW % 4 || K % 4) return MTR_E_SHAPE;
  if (B * HW > 0x7fffffffLL || (long long)K * HW > 0x7fffffffLL || (long long)M * HW > 0x7fffffffLL)
    return MTR_E_SHAPE;
  if (act < mtr::kActNone || act > mtr::kActHardswish) return MTR_E_PARAM;
  if (((uintptr_t)x % 16) || ((uintptr_t)weight % 16) || ((uintptr_t)y % 16) || ((uintptr_t)residual % 16))
    return MTR_E_ALIGN;
  if (x == y || (residual && residual == x)) return MTR_E_PARAM;  // y is written while x is still read
  if (B == 0) return MTR_OK;
  const float* xf = (const float*)x;
  const float* rf = (const float*)residual;
  float* yf = (float*)y;
  const long long n_total = B * HW;
  hipStream_t s = (hipStream_t)stream;
  const mtr::Conv1x1Plan p = mtr::pick_config(M, K, HW, B);
  switch (p.cfg) {
    case mtr::kCfgWide:
      return mtr::launch_conv1x1_cfg<2, 2, 3, 2, 16>(xf, weight, bias, gate, rf, yf, act, M, K, HW, n_total, s);
    case mtr::kCfgSquare:
      return mtr::launch_conv1x1_cfg<2, 2, 2, 2, 16>(xf, weight, bias, gate, rf, yf, act, M, K, HW, n_total, s);
    default:
      switch (p.waves_m) {
        case 1: return mtr::launch_conv1x1_cfg<1, 1, 1, 1, 16>(xf, weight, bias, gate, rf, yf, act, M, K, HW, n_total, s);
        case 2: return mtr::launch_conv1x1_cfg<2, 1, 1, 1, 16>(xf, weight, bias, gate, rf, yf, act, M, K, HW, n_total, s);
        case 3: return mtr::launch_conv1x1_cfg<3, 1, 1, 1, 16>(xf, weight, bias, gate, rf, yf, act, M, K, HW, n_total, s);
        case 4: return mtr::launch_conv1x1_cfg<4, 1, 1, 1, 32>(xf, weight, bias, gate, rf, yf, act, M, K, HW, n_total, s);
        default: return mtr::launch_conv1x1_cfg<5, 1, 1, 1, 16>(xf, weight, bias, gate, rf, yf, act, M, K, HW, n_total, s);
      }
  }
}
