// K18: depthwise 3x3 convolution, stride 1, zero padding 1, with the K10 epilogue (bias + activation, optionally
// the per-plane mean) in one pass over register blocks: K11's stride-1 block kernel (depthwise.hip) without its
// power-of-two assumptions, with the BITS of K11's generic kernel.
//
// K11's block kernel takes a plane only when W / 4 and H / 4 are powers of two and the plane has at most 64 blocks;
// every other plane (24x24 and 12x12 of the EfficientNetV2 family at 384 px, 128x128 and 64x64 of MobileNetV3 at
// 256 px) runs on its generic kernel, which is VALU-bound.  Here
//   - a lane owns a block of 4 rows x BC columns of outputs (BC = 4; for 16-bit tensors also 8: one 16-byte load per
//     row) and loads six aligned row vectors; everything stays in registers;
//   - the W / BC lanes of a plane row are padded to the next power of two LPR (1 .. 32), so a plane row never
//     straddles a 16-lane DPP row when LPR <= 16 and the halo columns come from row_shr:1 / row_shl:1; rows of 17 ..
//     32 blocks occupy 32 aligned lanes of one wave and take the halo by a wave shuffle.  Pad lanes load nothing,
//     store nothing and sum nothing;
//   - block rows are ceil(H / 4), any count; the last one may be partial (masked stores, masked sums);
//   - planes are packed into workgroups of 256 lanes by division; a plane of more than 256 lanes is walked in
//     passes by ONE workgroup, so a plane's mean never needs another workgroup, an atomic or a workspace.
//
// Arithmetic: per output acc = 0, fmaf over ky = 0..2 outer and kx = 0..2 inner, acc + bias, activate, settled(),
// one rounding -- depthwise3x3_kernel's, not the block kernel's (which seeds the accumulator with the bias).  The
// mean reproduces depthwise3x3_kernel's order as well: every group of four horizontally adjacent stored outputs is
// summed left to right; the group sums go to LDS (the only use of LDS), and lpp = min(64, next power of two >=
// groups) lanes per plane add groups s, s + 64, ... in ascending order and combine by the xor butterfly lpp / 2 .. 1.
// So a network may switch between K11's generic kernel and K18 per layer without changing a bit, and the bits do not
// depend on BC.
#include "common.h"

namespace mtr {

struct DwbGeom {
  int n_planes, C, H, W;
  int nbx;        // blocks per plane row = W / BC
  int lpr_log2;   // lanes per plane row = 1 << lpr_log2 >= nbx
  int lp;         // lanes per plane = ceil(H / 4) << lpr_log2
  int ppw;        // planes per workgroup (lp <= 256), else 1
  int passes;     // ceil(lp / 256) when one plane spans more than the workgroup, else 1
  int groups;     // groups of four outputs per plane = H * W / 4
  int lpp;        // lanes that finish one plane's mean (depthwise3x3_kernel's lpp)
  float inv_hw;
  FastDiv d_c, d_lp;
};

template <int CTRL>
__device__ __forceinline__ float dwb_row_shift(float v) {
  // row_shr:1 (0x111): lane i gets lane i - 1; row_shl:1 (0x101): lane i gets lane i + 1; bound_ctrl: lanes
  // without a source inside the 16-lane row get 0
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}

template <typename T, int ACT, int BC>
__global__ __launch_bounds__(256) void depthwise3x3_blocks_kernel(
    const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    T* __restrict__ y, float* __restrict__ row_mean, DwbGeom g) {
  static_assert(BC == 4 || (BC == 8 && sizeof(T) == 2), "4 columns, or 8 in 16 bits");
  struct alignas(BC * sizeof(T)) Vec { T v[BC]; };
  extern __shared__ float dwb_part[];  // [ppw][groups] group sums
  const int tid = (int)threadIdx.x;
  const int p0 = (int)blockIdx.x * g.ppw;
  const int W4 = g.W >> 2;
  for (int pass = 0; pass < g.passes; ++pass) {
    const int idx = pass * 256 + tid;
    const int q = (int)fastdiv((unsigned)idx, g.d_lp);
    const int local = idx - q * g.lp;
    const int by = local >> g.lpr_log2, bx = local & ((1 << g.lpr_log2) - 1);
    const int plane = p0 + q;
    // (q < ppw: the lanes behind the last whole plane of the workgroup; with passes > 1: behind the plane's end)
    const bool live = q < g.ppw && plane < g.n_planes && bx < g.nbx;
    const int p = live ? plane : 0;
    const int c = p - (int)fastdiv((unsigned)p, g.d_c) * g.C;
    const int oy0 = by << 2, ox0 = bx * BC;
    const T* xp = x + (size_t)p * (size_t)(g.H * g.W) + ox0;
    Vec raw[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      int iy = oy0 - 1 + r;
      iy = iy < 0 ? 0 : (iy >= g.H ? g.H - 1 : iy);  // clamped: rows outside the plane are zeroed below
      if (live) {
        raw[r] = *reinterpret_cast<const Vec*>(xp + iy * g.W);
      } else {
#pragma unroll
        for (int j = 0; j < BC; ++j) raw[r].v[j] = T(0.0f);
      }
    }
    float wk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = w[c * 9 + k];
    const float b = bias[c];
    const bool has_left = bx > 0, has_right = bx + 1 < g.nbx;
    float in[6][BC + 2];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const int iy = oy0 - 1 + r;
      const bool row_ok = iy >= 0 && iy < g.H;
#pragma unroll
      for (int j = 0; j < BC; ++j) in[r][1 + j] = row_ok ? to_f32(raw[r].v[j]) : 0.0f;
      float l, rgt;
      if (g.lpr_log2 <= 4) {  // (uniform) the plane row's lanes sit inside one DPP row
        l = dwb_row_shift<0x111>(in[r][BC]);
        rgt = dwb_row_shift<0x101>(in[r][1]);
      } else {  // 32 aligned lanes of one wave; the row's first / last lane is masked below
        l = __shfl_up(in[r][BC], 1, 64);
        rgt = __shfl_down(in[r][1], 1, 64);
      }
      in[r][0] = has_left ? l : 0.0f;
      in[r][BC + 1] = has_right ? rgt : 0.0f;
    }
    T* yp = y + (size_t)p * (size_t)(g.H * g.W) + oy0 * g.W + ox0;
    float* part = dwb_part + q * g.groups + oy0 * W4 + (ox0 >> 2);
#pragma unroll
    for (int orow = 0; orow < 4; ++orow) {
      float acc[BC];
#pragma unroll
      for (int o = 0; o < BC; ++o) acc[o] = 0.0f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int o = 0; o < BC; ++o) acc[o] = fmaf(in[orow + ky][o + kx], wk[ky * 3 + kx], acc[o]);
      Vec out;
      float gs[BC / 4];
#pragma unroll
      for (int h = 0; h < BC / 4; ++h) {
        float s = 0.0f;
#pragma unroll
        for (int o = 4 * h; o < 4 * h + 4; ++o) {
          const float a = settled(activate<ACT>(acc[o] + b));
          if constexpr (sizeof(T) == 4) out.v[o] = a; else out.v[o] = T(a);
          s += to_f32(out.v[o]);
        }
        gs[h] = s;
      }
      if (live && oy0 + orow < g.H) {
        *reinterpret_cast<Vec*>(yp + orow * g.W) = out;
        if (row_mean) {
#pragma unroll
          for (int h = 0; h < BC / 4; ++h) part[orow * W4 + h] = gs[h];
        }
      }
    }
  }
  if (!row_mean) return;  // (uniform)
  __syncthreads();
  // depthwise3x3_kernel's order: slot s of a plane adds its groups s, s + 64, ... from 0, then the butterfly.
  // Planes behind the tensor's end (last workgroup) read sums nobody wrote and store nothing.
  const int s = tid & (g.lpp - 1), per_pass = 256 / g.lpp;
  for (int base = 0; base < g.ppw; base += per_pass) {  // (uniform over the workgroup)
    const int q = base + tid / g.lpp;
    float sum = 0.0f;
    if (q < g.ppw && p0 + q < g.n_planes)
      for (int v = s; v < g.groups; v += 64) sum += dwb_part[q * g.groups + v];
    for (int m = g.lpp >> 1; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
    if (q < g.ppw && p0 + q < g.n_planes && s == 0) row_mean[p0 + q] = sum * g.inv_hw;
  }
}

// The planes K18 takes, for a layer with K11's stride and padding arguments: K11's argument errors first, in its
// order, then MTR_E_SHAPE for everything that K11 runs and this kernel does not.  (The dtype comes last, as in K11.)
static int dwb_check(int H, int W, int stride, int pad_top, int pad_left, int pad_bottom,
                     int pad_right) {
  if (H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (stride != 1 && stride != 2) return MTR_E_PARAM;
  if (pad_top < 0 || pad_top > 1 || pad_left < 0 || pad_left > 1 || pad_bottom < 0 || pad_bottom > 2 ||
      pad_right < 0 || pad_right > 2)
    return MTR_E_PARAM;
  if (stride != 1) return MTR_E_SHAPE;
  if (pad_top != 1 || pad_left != 1 || pad_bottom != 1 || pad_right != 1) return MTR_E_SHAPE;
  if (W % 4 != 0) return MTR_E_SHAPE;
  if (H > 128 || W > 128) return MTR_E_SHAPE;
  return MTR_OK;
}

// auto: 16-bit planes whose rows are whole 16-byte vectors take 4 x 8 blocks from 24 columns on -- measured faster
// or level at W = 24, 64 and 128 and 8 % slower at W = 8 and 16
static int dwb_auto_block_cols(int dtype, int W) { return (dtype != MTR_F32 && W % 8 == 0 && W >= 24) ? 8 : 4; }

template <typename T, int BC>
static int launch_depthwise_blocks(const void* x, const float* w, const float* bias, int act, void* y,
                                   float* row_mean, long long n_planes, int C, int H, int W,
                                   hipStream_t stream) {
  DwbGeom g;
  g.n_planes = (int)n_planes; g.C = C; g.H = H; g.W = W;
  g.nbx = W / BC;
  g.lpr_log2 = 0;
  while ((1 << g.lpr_log2) < g.nbx) ++g.lpr_log2;
  g.lp = ((H + 3) / 4) << g.lpr_log2;
  g.ppw = g.lp <= 256 ? 256 / g.lp : 1;
  if (g.ppw > n_planes) g.ppw = (int)n_planes;
  g.passes = g.lp <= 256 ? 1 : (g.lp + 255) / 256;
  g.groups = H * (W / 4);
  g.lpp = 1;
  while (g.lpp < 64 && g.lpp < g.groups) g.lpp <<= 1;
  g.inv_hw = 1.0f / (float)(H * W);
  g.d_c = make_fastdiv((unsigned)C);
  g.d_lp = make_fastdiv((unsigned)g.lp);
  const long long n_wg = (n_planes + g.ppw - 1) / g.ppw;
  const dim3 grid((unsigned)n_wg), block(256);
  const size_t lds = row_mean ? (size_t)g.ppw * g.groups * sizeof(float) : 0;  // <= 16 KiB (128 x 128)
  MTR_CLEAR_STALE();
  return dispatch_act(act, [&](auto tag) -> int {
    hipLaunchKernelGGL((depthwise3x3_blocks_kernel<T, decltype(tag)::value, BC>), grid, block, lds, stream,
                       (const T*)x, w, bias, (T*)y, row_mean, g);
    MTR_CHECK_LAUNCH();
    return MTR_OK;
  });
}

}  // namespace mtr

extern "C" int mtr_depthwise3x3_blocks_supported(int dtype, int H, int W, int stride, int pad_top, int pad_left,
                                                 int pad_bottom, int pad_right, int* block_cols) {
  if (!block_cols) return MTR_E_NULL;
  *block_cols = 0;
  const int rc = mtr::dwb_check(H, W, stride, pad_top, pad_left, pad_bottom, pad_right);
  if (rc != MTR_OK) return rc;
  if (dtype != MTR_F32 && dtype != MTR_F16 && dtype != MTR_BF16) return MTR_E_DTYPE;
  *block_cols = mtr::dwb_auto_block_cols(dtype, W);
  return MTR_OK;
}

extern "C" int mtr_depthwise3x3_blocks_bias_act_opts(const void* x, int dtype, const float* weight,
                                                     const float* bias, int act, long long B, int C, int H,
                                                     int W, void* y, float* row_mean, mtr_stream_t stream,
                                                     int block_cols) {
  if (!x || !weight || !bias || !y) return MTR_E_NULL;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (block_cols != 0 && block_cols != 4 && block_cols != 8) return MTR_E_PARAM;
  if (act < mtr::kActNone || act > mtr::kActHardswish) return MTR_E_PARAM;
  const int rc = mtr::dwb_check(H, W, 1, 1, 1, 1, 1);
  if (rc != MTR_OK) return rc;
  if (B * C >= (1LL << 24)) return MTR_E_SHAPE;
  if (block_cols == 8 && dtype == MTR_F32) return MTR_E_PARAM;  // a 4 x 8 block is one 16-byte load in 16 bits only
  if (block_cols == 8 && W % 8 != 0) return MTR_E_SHAPE;
  if ((uintptr_t)x % 16 || (uintptr_t)y % 16) return MTR_E_ALIGN;
  if (B == 0) return MTR_OK;
  const int bc = block_cols ? block_cols : mtr::dwb_auto_block_cols(dtype, W);
  hipStream_t s = (hipStream_t)stream;
  const long long n = B * C;
  switch (dtype) {
    case MTR_F32: return mtr::launch_depthwise_blocks<float, 4>(x, weight, bias, act, y, row_mean, n, C, H, W, s);
    case MTR_F16:
      return bc == 8 ? mtr::launch_depthwise_blocks<__half, 8>(x, weight, bias, act, y, row_mean, n, C, H, W, s)
                     : mtr::launch_depthwise_blocks<__half, 4>(x, weight, bias, act, y, row_mean, n, C, H, W, s);
    case MTR_BF16:
      return bc == 8 ? mtr::launch_depthwise_blocks<__hip_bfloat16, 8>(x, weight, bias, act, y, row_mean, n, C, H, W, s)
                     : mtr::launch_depthwise_blocks<__hip_bfloat16, 4>(x, weight, bias, act, y, row_mean, n, C, H, W, s);
    default: return MTR_E_DTYPE;
  }
}

extern "C" int mtr_depthwise3x3_blocks_bias_act(const void* x, int dtype, const float* weight, const float* bias,
                                                int act, long long B, int C, int H, int W, void* y,
                                                float* row_mean, mtr_stream_t stream) {
  return mtr_depthwise3x3_blocks_bias_act_opts(x, dtype, weight, bias, act, B, C, H, W, y, row_mean, stream, 0);
}
