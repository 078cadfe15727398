// What K25h (expand_dw16.hip), K26h (expand_dw16_planes.hip) and K27h (expand_dw16_tiles.hip) share: the 1x1 expand
// convolution of an MBConv block and the depthwise 3x3 convolution behind it, f16 / bf16, in ONE launch, the expanded
// activation kept in LDS.  Per image b (stride s = 1 but in K27h; the mean in K25h and K26h alone):
//
//   mid[b, c, p] = rnd16(act1(bias1[c] + sum_k W1[c, k] * x[b, k, p]))                                    c < Cmid
//   y[b, c, o]   = rnd16(act2(dw(bias2[c], Wd[c], the 3x3 window of mid[b, c] around s * o)))
//   mean[b, c]   = (1 / HW) * sum_p f32(y[b, c, p])                                                      (optional)
//
// where dw is K11's f32 arithmetic for the plane, and the order matters to the bits: the accumulator started at the
// bias and nine fmaf (K25h, K11's block kernel), or nine fmaf from 0.0f and the bias added last (K26h, K27h: K11's
// generic kernel); each file says which.  The result has the BITS of the two-kernel chain K13h (conv1x1_16.hip) + K11
// (depthwise.hip).  A workgroup of four waves owns CM expanded channels of one image over a span of positions (the
// plane, or K27h's band of rows):
//
//   phase 1  K13h's GEMM for the slice, Y^T = X^T W^T on v_mfma_f32_32x32x16_{f16,bf16}: the same 16-k steps at
//            k = 0, 16, 32, ..., lane (r, h) holding the 8-k group 2 step + h, k past Cin and positions past the span
//            zero-filled, the X^T image staged through LDS in k-tiles of 32 by loader units of 4 k x 8 positions, the
//            weight fragments as 16-byte loads from global memory one k-tile ahead.  K13h's bits do not depend on the
//            tile, so each kernel cuts its span into the 32-position tiles that suit it (its EdwPlaneTiles /
//            EdtBandTiles).  Bias, activation (f32) and ONE plain-cast rounding in registers; `settled` keeps the
//            activation's last product an f32 value of its own, as K13h's stored output is.
//   between  the X^T image is dead: the same LDS becomes the slice's image [c][rows][LW] inside a ring of zeros, zeroed
//            first, so phase 2 needs no bounds test.
//   phase 2  each kernel's own (K11's block arithmetic, K11's generic walk with the mean, K27h's segments): in its file.
//
// K28h (expand_dw16_k5.hip) builds the same pair for the depthwise 5x5 layers (K15's arithmetic and mean, stride 1 or 2)
// from the same pieces: phase 1 as edw_gemm_span in passes over the plane, the image beside the staging buffers.
//
// No atomics, no split-K, no workspace: the same inputs give the same bits.
#pragma once
#include "common.h"

namespace mtr {

typedef float edw_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short edw_u16x8 __attribute__((ext_vector_type(8)));

template <int DT> struct EdwBits;
template <> struct EdwBits<MTR_F16> {
  typedef __half T;  // K11's element type: phase 2 rounds and widens exactly as depthwise.hip does
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
  static __device__ __forceinline__ edw_f32x16 mfma(uint4 a, uint4 b, edw_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};
template <> struct EdwBits<MTR_BF16> {
  typedef __hip_bfloat16 T;
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
  static __device__ __forceinline__ edw_f32x16 mfma(uint4 a, uint4 b, edw_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};

constexpr int kEdwBK = 32;               // k-tile of the X^T image
constexpr int kEdwKS = kEdwBK / 16;      // its 16-k steps
constexpr int kEdwLDK = kEdwBK + 8;      // its row (one position), padded like K13h's (K27h: a run-time ldk)
constexpr int kEdwColPad = 4;            // image column j of the slice's image sits at index j + 4 (K27h: its own)
constexpr size_t kEdwMaxLds = 160 * 1024;

// ---- phase 1, piece by piece

// The X^T image of one k-tile on its way from global memory to LDS: thread tid owns the loader units tid, tid + 256, ...
// of 4 k x 8 positions, BN staged positions.
template <int BN> struct EdwXTile {
  static constexpr int UNITS = (kEdwBK / 4) * (BN / 8);
  static constexpr int NU = (UNITS + 255) / 256;  // units per loader thread
  edw_u16x8 xr[NU][4];

  // k0 .. k0 + 31 of the positions 0 .. n_pos - 1 behind xb (n_pos % 8 == 0: a unit is inside the span or past it)
  __device__ __forceinline__ void load(const unsigned short* xb, int tid, int k0, int K, int HW, int n_pos) {
#pragma unroll
    for (int n = 0; n < NU; ++n) {
      const int u = tid + 256 * n;
      const int p8 = u % (BN / 8), k4 = u / (BN / 8);
      const bool on = u < UNITS && 8 * p8 < n_pos;
      const unsigned short* src = xb + 8 * p8;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = k0 + 4 * k4 + i;
        edw_u16x8 t = (edw_u16x8)0;
        if (on && k < K) t = __builtin_bit_cast(edw_u16x8, *reinterpret_cast<const uint4*>(src + (long long)k * HW));
        xr[n][i] = t;
      }
    }
  }
  // 4 k-rows x 8 positions -> 8 positions x 4 k of the image xs[BN][ldk]; live(p8, k4): the units the image has
  template <class Live>
  __device__ __forceinline__ void store(unsigned short* xs, int ldk, int tid, Live live) const {
#pragma unroll
    for (int n = 0; n < NU; ++n) {
      const int u = tid + 256 * n;
      const int p8 = u % (BN / 8), k4 = u / (BN / 8);
      if (u < UNITS && live(p8, k4)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          uint2 v;
          v.x = (unsigned)xr[n][0][j] | ((unsigned)xr[n][1][j] << 16);
          v.y = (unsigned)xr[n][2][j] | ((unsigned)xr[n][3][j] << 16);
          *reinterpret_cast<uint2*>(&xs[(8 * p8 + j) * ldk + 4 * k4]) = v;
        }
      }
    }
  }
};

// a lane's weight fragments of the k-tile at k0: rows mrow + 32 i, k 16 s + 8 h .. + 7
template <int FM>
__device__ __forceinline__ void edw_load_w(uint4 (&wr)[FM][kEdwKS], const unsigned short* w1, int mrow, int M, int K,
                                           int k0, int h) {
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = mrow + 32 * i;
#pragma unroll
    for (int s = 0; s < kEdwKS; ++s) {
      const int k = k0 + 16 * s + 8 * h;
      uint4 t = make_uint4(0u, 0u, 0u, 0u);
      if (m < M && k < K) t = *reinterpret_cast<const uint4*>(w1 + (long long)m * K + k);
      wr[i][s] = t;
    }
  }
}

template <int FM, int FN>
__device__ __forceinline__ void edw_clear(edw_f32x16 (&acc)[FM][FN]) {
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
}

// The 32-position tiles of a wave: tile j starts pos(j) positions into the span.  K25h and K26h: FN tiles in a row
// from `first`, every tile and every 16-k step run.  (K27h's EdtBandTiles skips what lies past the band.)
struct EdwPlaneTiles {
  int first;
  __device__ __forceinline__ int pos(int j) const { return first + 32 * j; }
  __device__ __forceinline__ bool step(int) const { return true; }
  __device__ __forceinline__ bool tile(int) const { return true; }
};

// the MFMAs of one k-tile; xa: this lane's k-group of position r of the image, &xs[r * ldk + 8 * h]
template <class Hh, int FM, int FN, class Tiles>
__device__ __forceinline__ void edw_mfma_ktile(edw_f32x16 (&acc)[FM][FN], const uint4 (&wc)[FM][kEdwKS],
                                               const unsigned short* xa, int ldk, Tiles tiles) {
#pragma unroll
  for (int s = 0; s < kEdwKS; ++s) {
    if (!tiles.step(s)) continue;
    uint4 a[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j)
      if (tiles.tile(j)) a[j] = *reinterpret_cast<const uint4*>(xa + tiles.pos(j) * ldk + 16 * s);
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        if (tiles.tile(j)) acc[i][j] = Hh::mfma(a[j], wc[i][s], acc[i][j]);
  }
}

// conv1x1_16_kernel's loop over a span of one image's plane, positions 0 .. n_pos - 1 behind xb (past n_pos:
// zero-filled; HW: the plane, a channel's stride), through two buffers xs[2][BN * kEdwLDK]: the next k-tile's loads are
// in flight during this one's MFMAs.  Ends on a barrier: the buffers are free.  (K27h, one buffer of a run-time ldk,
// runs its own loop of the same pieces.)
template <class Hh, int BN, int FM, int FN, class Tiles>
__device__ __forceinline__ void edw_gemm_span(edw_f32x16 (&acc)[FM][FN], unsigned short* xs, const unsigned short* xb,
                                              const unsigned short* w1, int mrow, int M, int K, int HW, int n_pos,
                                              int tid, Tiles tiles) {
  constexpr int BK = kEdwBK, LDK = kEdwLDK, KS = kEdwKS;
  const int r = tid & 31, h = (tid & 63) >> 5;
  const auto all = [](int, int) { return true; };
  EdwXTile<BN> xt;
  edw_clear(acc);
  uint4 wc[FM][KS], wnx[FM][KS];
  const int n_tiles = (K + BK - 1) / BK;
  xt.load(xb, tid, 0, K, HW, n_pos);
  edw_load_w(wc, w1, mrow, M, K, 0, h);
  xt.store(xs, LDK, tid, all);
  __syncthreads();
  for (int t = 0; t < n_tiles; ++t) {
    const int buf = t & 1;
    if (t + 1 < n_tiles) {  // in flight during this tile's MFMAs
      xt.load(xb, tid, (t + 1) * BK, K, HW, n_pos);
      edw_load_w(wnx, w1, mrow, M, K, (t + 1) * BK, h);
    }
    edw_mfma_ktile<Hh>(acc, wc, &xs[buf * (BN * LDK) + r * LDK + 8 * h], LDK, tiles);
    if (t + 1 < n_tiles) {
      xt.store(xs + (buf ^ 1) * (BN * LDK), LDK, tid, all);  // the other buffer: last read before the previous barrier
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int s = 0; s < KS; ++s) wc[i][s] = wnx[i][s];
    }
    __syncthreads();
  }
}

// the same over the whole plane of one image (K25h, K26h)
template <class Hh, int BN, int FM, int FN>
__device__ __forceinline__ void edw_gemm_plane(edw_f32x16 (&acc)[FM][FN], unsigned short* xs, const unsigned short* xb,
                                               const unsigned short* w1, int mrow, int M, int K, int HW, int tid,
                                               EdwPlaneTiles tiles) {
  edw_gemm_span<Hh, BN>(acc, xs, xb, w1, mrow, M, K, HW, HW, tid, tiles);
}

// ---- between the phases

// The slice's image ms[CM][plane] of rows of LW elements: image row 0 is row `row0` of the plane (a ring row where that
// is -1), column j of the plane sits at index col_pad + j.
struct EdwImage {
  unsigned short* ms;
  int plane, LW, row0, col_pad;
};

// zeros all of it, ring and dead channels included (n = CM * plane elements, a multiple of 8: whole 16-byte groups)
__device__ __forceinline__ void edw_zero_image(unsigned short* ms, int n, int tid) {
  const int n16 = n >> 3;
  for (int i = tid; i < n16; i += 256) reinterpret_cast<uint4*>(ms)[i] = make_uint4(0u, 0u, 0u, 0u);
}

// K13h's epilogue into the image: the lane holds the channels cl + 32 i of the slice (m0 + cl + 32 i of the layer) and
// the positions p_first + tiles.pos(j) + 8 q + 4 h + 0 .. 3 of each tile -- inside one row of the plane (W % 4 == 0,
// p_first % 4 == 0).  Those in [p_lo, p_hi) are stored; rowcol(p, row, col) says where a position lies.
template <class Hh, int FM, int FN, class Tiles, class RowCol>
__device__ __forceinline__ void edw_store_expanded(const edw_f32x16 (&acc)[FM][FN], int act1,
                                                   const float* __restrict__ bias1, int m0, int M, int cl, int h,
                                                   Tiles tiles, int p_first, int p_lo, int p_hi, RowCol rowcol,
                                                   EdwImage im) {
  with_act(act1, [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int c = cl + 32 * i;
      if (m0 + c >= M) continue;
      const float bm = bias1[m0 + c];
#pragma unroll
      for (int j = 0; j < FN; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int p = p_first + tiles.pos(j) + 8 * q + 4 * h;
          if (p < p_lo || p >= p_hi) continue;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = settled(activate<ACT>(acc[i][j][4 * q + e] + bm));
          uint2 o;
          o.x = (unsigned)Hh::rnd(v[0]) | ((unsigned)Hh::rnd(v[1]) << 16);
          o.y = (unsigned)Hh::rnd(v[2]) | ((unsigned)Hh::rnd(v[3]) << 16);
          int row, col;
          rowcol(p, row, col);
          *reinterpret_cast<uint2*>(&im.ms[c * im.plane + (row - im.row0) * im.LW + im.col_pad + col]) = o;
        }
      }
    }
  });
}

// K25h's and K26h's workgroup-to-image mapping.  Every workgroup of an image re-reads that image's x from L2, and
// workgroups are dealt round-robin over the 8 XCDs: with xcd_map the image index comes from blockIdx.x % 8 and
// blockIdx.x / (8 chunks), so the chunks of one image land on one XCD and x crosses to one L2; without it blockIdx.x =
// image * chunks + chunk.  The bits do not depend on it.  (xcd_map rounds the images up to 8: the workgroups of
// b >= B leave, whole, before any barrier.)
__device__ __forceinline__ void edw_image_chunk(int xcd_map, int chunks, int& b, int& chunk) {
  if (xcd_map) {
    const int q = (int)blockIdx.x >> 3;
    b = (q / chunks) * 8 + ((int)blockIdx.x & 7);
    chunk = q % chunks;
  } else {
    b = (int)blockIdx.x / chunks;
    chunk = (int)blockIdx.x % chunks;
  }
}

// ---- host

static int edw_ilog2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

// launch_depthwise's condition for K11's stride-1 block kernel (depthwise.hip), restated for a 16-byte aligned x.
// max_lp_log2 6: all of them; 4: those of up to 256 positions, K25h's
static bool edw_k11_block_plane(int H, int W, int max_lp_log2 = 6) {
  if (H % 4 || W % 4) return false;
  const int tw = edw_ilog2_exact(W / 4), th = edw_ilog2_exact(H / 4);
  return tw >= 0 && tw <= 4 && th >= 0 && tw + th <= max_lp_log2;
}

struct EdwArgs {
  const void *x, *w1;
  const float *bias1, *wd, *bias2;
  void* y;
  float* row_mean;  // (K27h: none)
  int act1, act2;
  long long B;
  hipStream_t stream;
};

// The refusals of an entry up to the launch, in their order: MTR_E_NULL, MTR_E_DTYPE, the entry's own shape(hw_in,
// hw_out) (MTR_E_SHAPE; it names the positions of an input and an output plane), the activation codes and `mapping`
// (-1 .. 1; MTR_E_PARAM), MTR_E_ALIGN, and y overlapping x (MTR_E_PARAM: y is written while other workgroups still
// read x).
template <class Shape>
static int edw_check(const EdwArgs& a, int dtype, int Cin, int Cmid, int mapping, Shape&& shape) {
  if (!a.x || !a.w1 || !a.bias1 || !a.wd || !a.bias2 || !a.y) return MTR_E_NULL;
  if (dtype != MTR_F16 && dtype != MTR_BF16) return MTR_E_DTYPE;
  int hw_in = 0, hw_out = 0;
  const int e = shape(hw_in, hw_out);
  if (e != MTR_OK) return e;
  if (a.act1 < kActNone || a.act1 > kActHardswish || a.act2 < kActNone || a.act2 > kActHardswish) return MTR_E_PARAM;
  if (mapping < -1 || mapping > 1) return MTR_E_PARAM;
  if (((uintptr_t)a.x % 16) || ((uintptr_t)a.w1 % 16) || ((uintptr_t)a.y % 16) || ((uintptr_t)a.bias1 % 4) ||
      ((uintptr_t)a.wd % 4) || ((uintptr_t)a.bias2 % 4) || ((uintptr_t)a.row_mean % 4))
    return MTR_E_ALIGN;
  const uintptr_t xb = (uintptr_t)a.x, yb = (uintptr_t)a.y;
  const uintptr_t xn = (uintptr_t)a.B * Cin * hw_in * 2, yn = (uintptr_t)a.B * Cmid * hw_out * 2;
  if (a.x == a.y || (xb < yb + yn && yb < xb + xn)) return MTR_E_PARAM;
  return MTR_OK;
}

// One configuration's launch: the LDS is the larger of the X^T image and the slice's image, at most kEdwMaxLds
// (MTR_E_SHAPE), the grid gx workgroups (MTR_E_SHAPE past 2^31 - 1).  a.y == NULL is the shape query: -> the bytes of
// LDS, no launch.  launch(grid, lds) is the hipLaunchKernelGGL of `kern`.
template <class Launch>
static int edw_launch(const void* kern, const EdwArgs& a, size_t xs_bytes, size_t ms_bytes, long long gx,
                      Launch&& launch) {
  const size_t lds = xs_bytes > ms_bytes ? xs_bytes : ms_bytes;
  if (lds > kEdwMaxLds) return MTR_E_SHAPE;
  if (gx > 0x7fffffffLL) return MTR_E_SHAPE;
  if (!a.y) return (int)lds;
  if (lds > 64 * 1024) {
    const int e = allow_dynamic_lds(kern, kEdwMaxLds);
    if (e != MTR_OK) return e;
  }
  MTR_CLEAR_STALE();
  launch(dim3((unsigned)gx), lds);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

}  // namespace mtr
