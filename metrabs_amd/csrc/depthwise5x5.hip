// K15: depthwise 5x5 convolution with the K10 epilogue (bias + activation, optionally the per-plane
// mean for the squeeze-excite block behind it) in one pass, NCHW: K11's contract for the 5x5 layers
// of MobileNetV3-Large (and of the EfficientNet-B family, efficientnet.py:389-395).
//
// Like K10 / K11 this sits outside the reference's hot path: it serves the PyTorch-ROCm backbone's
// inference copy (backbones.fold_batchnorm(fused_epilogue=True)), where these layers otherwise run
// on PyTorch's generic depthwise kernel followed by K10's in-place pass over the output.
//
// A lane that took its 5x5 window straight from memory would need an 8x8 (stride 1, 4x4 outputs) or
// 11x11 (stride 2) window with halo columns on BOTH sides of every aligned vector, and four kinds of
// padding to mask.  Here a workgroup stages whole (b, c) planes into LDS instead, as f32, into tiles
// that carry the zero padding: the planes of a group are contiguous in memory, so the copy is one
// flat run of aligned 4-element vectors (or of single elements when the base or the row length is
// not aligned -- the only place the two paths differ).  The tiles' borders are zeroed once per
// workgroup; the grid is persistent and the copies only ever overwrite the interior.  Every lane
// then computes a block of RB x 4 outputs (4x4 at stride 1, 2x4 at stride 2) from aligned
// ds_read_b128 rows of its window: no bounds test, no select, no index arithmetic per tap.
//
// ONE arithmetic for every path: acc = 0, fma over (ky, kx) with ky outer, + bias, activation, one
// rounding; the per-plane sum is taken over the rounded outputs in an order that depends on the
// geometry alone (unit partial sums in LDS, a strided sum per lane, an xor butterfly), without
// atomics.  Aligned or unaligned base, first call or graph replay: the same bits.
#include "common.h"

namespace mtr {

struct Dw5Geom {
  int n_planes, C, H, W, OH, OW;
  int pt, pl;      // top / left zero padding (bottom / right follow from OH, OW)
  int PH, PW;      // LDS tile: rows, row stride in floats (a multiple of 4)
  int tile;        // PH * PW
  int ppb;         // planes per group (one pass of a workgroup)
  int UW, units;   // units (RB x 4 output blocks) per plane row / per plane
  int n_groups;
  int G;           // lanes that reduce one plane's sum (a power of two <= 64)
  float inv_hw;
  FastDiv d_c, d_units, d_uw, d_hw, d_w;  // d_hw, d_w: in vectors on the aligned path, else elements
};

constexpr int kDw5WeightSlot = 28;  // 25 taps + the bias, padded to whole float4

template <typename T, int ACT, int STRIDE>
__global__ __launch_bounds__(256) void depthwise5x5_kernel(
    const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
    T* __restrict__ y, float* __restrict__ row_mean, Dw5Geom g, int vec) {
  constexpr int RB = STRIDE == 1 ? 4 : 2;       // output rows of a unit
  constexpr int NR = (RB - 1) * STRIDE + 5;      // input rows of its window
  constexpr int NV = (3 * STRIDE + 5 + 3) / 4;   // aligned float4 per window row (8 / 11 columns)
  extern __shared__ float4 dw5_smem[];
  float* tiles = reinterpret_cast<float*>(dw5_smem);
  float* wts = tiles + g.ppb * g.tile;
  float* partial = wts + g.ppb * kDw5WeightSlot;
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  for (int i = tid; i < (g.ppb * g.tile) >> 2; i += nt) dw5_smem[i] = float4{0.0f, 0.0f, 0.0f, 0.0f};
  __syncthreads();
  for (int grp = (int)blockIdx.x; grp < g.n_groups; grp += (int)gridDim.x) {
    const int p0 = grp * g.ppb;
    const int np = g.n_planes - p0 < g.ppb ? g.n_planes - p0 : g.ppb;
    for (int i = tid; i < np * 26; i += nt) {
      const int q = i / 26, k = i - q * 26;
      const unsigned p = (unsigned)(p0 + q);
      const int c = (int)(p - fastdiv(p, g.d_c) * (unsigned)g.C);
      wts[q * kDw5WeightSlot + k] = k < 25 ? w[c * 25 + k] : bias[c];
    }
    const T* xg = x + (size_t)p0 * (size_t)(g.H * g.W);
    if (vec) {
      const int n4 = (np * g.H * g.W) >> 2;
#pragma unroll 2
      for (int i = tid; i < n4; i += nt) {
        float f[4];
        load_vec<T, 4>(xg + 4 * i, f);
        const int q = (int)fastdiv((unsigned)i, g.d_hw);
        const int r = i - q * (int)g.d_hw.d;
        const int iy = (int)fastdiv((unsigned)r, g.d_w);
        const int ix = (r - iy * (int)g.d_w.d) << 2;
        float* d = tiles + q * g.tile + (iy + g.pt) * g.PW + ix + g.pl;
        d[0] = f[0]; d[1] = f[1]; d[2] = f[2]; d[3] = f[3];
      }
    } else {
      const int n = np * g.H * g.W;
#pragma unroll 4
      for (int i = tid; i < n; i += nt) {
        const float f = to_f32(xg[i]);
        const int q = (int)fastdiv((unsigned)i, g.d_hw);
        const int r = i - q * (int)g.d_hw.d;
        const int iy = (int)fastdiv((unsigned)r, g.d_w);
        const int ix = r - iy * (int)g.d_w.d;
        tiles[q * g.tile + (iy + g.pt) * g.PW + ix + g.pl] = f;
      }
    }
    __syncthreads();
    // planes past the end of the tensor (last group) are computed on stale tiles and not stored
    for (int u = tid; u < g.ppb * g.units; u += nt) {
      const int q = (int)fastdiv((unsigned)u, g.d_units);
      const int v = u - q * g.units;
      const int uy = (int)fastdiv((unsigned)v, g.d_uw);
      const int oy0 = uy * RB, ox0 = (v - uy * g.UW) << 2;
      float wk[kDw5WeightSlot];
#pragma unroll
      for (int k = 0; k < kDw5WeightSlot / 4; ++k) {
        const float4 t = reinterpret_cast<const float4*>(wts + q * kDw5WeightSlot)[k];
        wk[4 * k] = t.x; wk[4 * k + 1] = t.y; wk[4 * k + 2] = t.z; wk[4 * k + 3] = t.w;
      }
      const float* win = tiles + q * g.tile + oy0 * STRIDE * g.PW + ox0 * STRIDE;
      float acc[RB][4];
#pragma unroll
      for (int a = 0; a < RB; ++a)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[a][o] = 0.0f;
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        float in[NV * 4];
#pragma unroll
        for (int n = 0; n < NV; ++n) {
          const float4 t = reinterpret_cast<const float4*>(win + r * g.PW)[n];
          in[4 * n] = t.x; in[4 * n + 1] = t.y; in[4 * n + 2] = t.z; in[4 * n + 3] = t.w;
        }
#pragma unroll
        for (int a = 0; a < RB; ++a) {
          const int ky = r - a * STRIDE;  // (compile-time after unrolling)
          if (ky < 0 || ky > 4) continue;
#pragma unroll
          for (int kx = 0; kx < 5; ++kx)
#pragma unroll
            for (int o = 0; o < 4; ++o) acc[a][o] = fmaf(in[o * STRIDE + kx], wk[ky * 5 + kx], acc[a][o]);
        }
      }
      const bool live = q < np;
      T* yp = y + (size_t)(p0 + (live ? q : 0)) * (size_t)(g.OH * g.OW) + ox0;
      float sum = 0.0f;
#pragma unroll
      for (int a = 0; a < RB; ++a) {
        struct alignas(4 * sizeof(T)) Out4 { T v[4]; } out;
        const bool row_ok = oy0 + a < g.OH;
        float s = 0.0f;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const float e = activate<ACT>(acc[a][o] + wk[25]);
          if constexpr (sizeof(T) == 4) out.v[o] = e; else out.v[o] = T(e);
          s += to_f32(out.v[o]);
        }
        if (row_ok) sum += s;
        if (live && row_ok) {
          if constexpr (sizeof(T) == 4)
            *reinterpret_cast<float4*>(yp + (oy0 + a) * g.OW) = float4{out.v[0], out.v[1], out.v[2], out.v[3]};
          else
            *reinterpret_cast<Out4*>(yp + (oy0 + a) * g.OW) = out;
        }
      }
      partial[u] = sum;
    }
    __syncthreads();
    if (row_mean) {
      const int l = tid & (g.G - 1), per_pass = nt / g.G;
      for (int base = 0; base < g.ppb; base += per_pass) {  // (uniform over the workgroup)
        const int q = base + tid / g.G;
        float s = 0.0f;
        if (q < g.ppb)
          for (int i = l; i < g.units; i += g.G) s += partial[q * g.units + i];
        for (int m = g.G >> 1; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
        if (q < np && l == 0) row_mean[p0 + q] = s * g.inv_hw;
      }
    }
    // (the next pass writes the weights and tiles, which nobody reads any more, and `partial` only
    // behind its own barrier)
  }
}

template <typename T, int STRIDE>
static int launch_depthwise5x5(const void* x, const float* w, const float* bias, int act, void* y,
                               float* row_mean, long long n_planes, int C, int H, int W, int OH, int OW,
                               int pt, int pl, int pb, int pr, hipStream_t stream) {
  constexpr int RB = STRIDE == 1 ? 4 : 2;
  if (n_planes >= (1LL << 30)) return MTR_E_SHAPE;
  // a padded plane of at most 112 x 112: its f32 tile, weights and unit sums fit 64 KiB of LDS
  if (H + pt + pb > 112 || W + pl + pr > 112) return MTR_E_SHAPE;
  Dw5Geom g;
  g.n_planes = (int)n_planes; g.C = C; g.H = H; g.W = W; g.OH = OH; g.OW = OW; g.pt = pt; g.pl = pl;
  const int UH = (OH + RB - 1) / RB;
  g.UW = OW / 4;
  g.units = UH * g.UW;
  const int rows = (UH * RB - 1) * STRIDE + 5, cols = STRIDE * OW + 4;  // what the windows read
  g.PH = rows > H + pt + pb ? rows : H + pt + pb;
  g.PW = ((cols > W + pl + pr ? cols : W + pl + pr) + 3) & ~3;
  g.tile = g.PH * g.PW;
  const int per_plane = (g.tile + kDw5WeightSlot + g.units) * 4;
  if (per_plane > 64 * 1024) return MTR_E_SHAPE;  // (not reached inside the 112 x 112 bound)
  // planes per group: enough units for 256 lanes inside 32 KiB of LDS (4 - 8 workgroups per CU).  (Measured, not
  // adopted yet: 64 planes of 8x8 per group, 45 KB, run in 52 instead of 70 us at batch 320)
  int ppb = (256 + g.units - 1) / g.units;
  if (ppb * per_plane > 32 * 1024) ppb = 32 * 1024 / per_plane;
  if (ppb < 1) ppb = 1;
  if (ppb > n_planes) ppb = (int)n_planes;
  g.ppb = ppb;
  g.n_groups = (int)((n_planes + ppb - 1) / ppb);
  g.G = 1;
  while (g.G < 64 && g.G < g.units) g.G <<= 1;
  g.inv_hw = 1.0f / (float)(OH * OW);
  const bool vec = (W & 3) == 0 && ((uintptr_t)x % (4 * sizeof(T))) == 0;
  g.d_c = make_fastdiv((unsigned)C);
  g.d_units = make_fastdiv((unsigned)g.units);
  g.d_uw = make_fastdiv((unsigned)g.UW);
  g.d_hw = make_fastdiv((unsigned)(vec ? H * W / 4 : H * W));
  g.d_w = make_fastdiv((unsigned)(vec ? W / 4 : W));
  int threads = (ppb * g.units + 63) & ~63;
  if (threads > 256) threads = 256;
  const size_t lds = (size_t)ppb * per_plane;
  // persistent grid: 256 CUs x as many workgroups as LDS and 2048 lanes per CU hold
  int per_cu = (int)(160 * 1024 / lds);
  if (per_cu > 2048 / threads) per_cu = 2048 / threads;
  if (per_cu < 1) per_cu = 1;
  int blocks = g.n_groups < 256 * per_cu ? g.n_groups : 256 * per_cu;
  const dim3 grid((unsigned)blocks), block((unsigned)threads);
  MTR_CLEAR_STALE();
  return dispatch_act(act, [&](auto tag) -> int {
    hipLaunchKernelGGL((depthwise5x5_kernel<T, decltype(tag)::value, STRIDE>), grid, block, lds, stream, (const T*)x,
                       w, bias, (T*)y, row_mean, g, vec ? 1 : 0);
    MTR_CHECK_LAUNCH();
    return MTR_OK;
  });
}

template <typename T>
static int dispatch_depthwise5x5(const void* x, const float* w, const float* bias, int act, void* y,
                                 float* row_mean, long long n_planes, int C, int H, int W, int OH, int OW,
                                 int stride, int pt, int pl, int pb, int pr, hipStream_t stream) {
  if (stride == 1)
    return launch_depthwise5x5<T, 1>(x, w, bias, act, y, row_mean, n_planes, C, H, W, OH, OW, pt, pl, pb, pr,
                                     stream);
  return launch_depthwise5x5<T, 2>(x, w, bias, act, y, row_mean, n_planes, C, H, W, OH, OW, pt, pl, pb, pr,
                                   stream);
}

}  // namespace mtr

extern "C" int mtr_depthwise5x5_bias_act_padded(const void* x, int dtype, const float* weight,
                                                const float* bias, int act, long long B, int C, int H,
                                                int W, int stride, int pad_top, int pad_left,
                                                int pad_bottom, int pad_right, void* y, float* row_mean,
                                                mtr_stream_t stream) {
  if (!x || !weight || !bias || !y) return MTR_E_NULL;
  if (B < 0 || C <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (stride != 1 && stride != 2) return MTR_E_PARAM;
  if (pad_top < 0 || pad_top > 2 || pad_left < 0 || pad_left > 2 || pad_bottom < 0 || pad_bottom > 3 ||
      pad_right < 0 || pad_right > 3)
    return MTR_E_PARAM;
  if (H + pad_top + pad_bottom < 5 || W + pad_left + pad_right < 5) return MTR_E_SHAPE;
  const int OH = (H + pad_top + pad_bottom - 5) / stride + 1, OW = (W + pad_left + pad_right - 5) / stride + 1;
  if (OW % 4 != 0) return MTR_E_SHAPE;
  if ((uintptr_t)y % 16) return MTR_E_ALIGN;
  if (B == 0) return MTR_OK;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case MTR_F32: return mtr::dispatch_depthwise5x5<float>(x, weight, bias, act, y, row_mean, B * C, C, H, W, OH, OW, stride, pad_top, pad_left, pad_bottom, pad_right, s);
    case MTR_F16: return mtr::dispatch_depthwise5x5<__half>(x, weight, bias, act, y, row_mean, B * C, C, H, W, OH, OW, stride, pad_top, pad_left, pad_bottom, pad_right, s);
    case MTR_BF16: return mtr::dispatch_depthwise5x5<__hip_bfloat16>(x, weight, bias, act, y, row_mean, B * C, C, H, W, OH, OW, stride, pad_top, pad_left, pad_bottom, pad_right, s);
    default: return MTR_E_DTYPE;
  }
}
