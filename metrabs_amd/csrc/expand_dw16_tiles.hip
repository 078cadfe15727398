// K27h: the 1x1 expand convolution of an MBConv block and the depthwise 3x3 convolution behind it (stride 1 or 2,
// padding 1, f16 / bf16) in ONE launch on the LARGE planes K25h (expand_dw16.hip) and K26h (expand_dw16_planes.hip)
// refuse -- 64x64, 128x128 -> 64x64, 32x32 -> 16x16 of MobileNetV3's early blocks -- where the expanded activation
// written by K13h and read straight back by K11 is nearly all of the chain's traffic.  There is no squeeze-excite
// mean: without it an output needs only its 3x3 window of the expanded activation, so a workgroup owns a BAND of
// output rows instead of the whole plane and recomputes the halo rows of the expand.
//
// Not part of the reference's hot path (like K10 - K26h): backbones.fold_batchnorm(dtype=f16 / bf16,
// fuse_expand_depthwise_tiles=True).  Per image b, stride s:
//
//   mid[b, c, p] = rnd16(act1(bias1[c] + sum_k W1[c, k] * x[b, k, p]))                                    c < Cmid
//   y[b, c, o]   = rnd16(act2(sum_{ky, kx} Wd[c, ky, kx] * mid[b, c, s * o + (ky - 1, kx - 1)] + bias2[c]))
//
// with the BITS of conv1x1_16_kernel (K13h) followed by depthwise3x3_kernel (K11's generic kernel, dw_finish).  A
// workgroup of four waves owns (image, chunk of 32 expanded channels, band of R output rows):
//
//   phase 1  K13h's GEMM as K25h / K26h run it (16-k steps at k = 0, 16, ... on v_mfma_f32_32x32x16_{f16,bf16}, the
//            same lane-to-k grouping and operand roles, k past Cin and positions past the band zero-filled; bias +
//            activation in f32, one plain-cast rounding behind `settled`) over the s R + 3 - s input rows of the band,
//            a contiguous span of positions of the plane (from the 16-byte boundary at or below its first row).
//            K13h's bits do not depend on the tile.  The X^T image of a k-tile of 32 sits in ONE LDS buffer (the
//            expands this kernel is for have one or two k-tiles); the next tile's global loads are in flight during
//            the MFMAs.  Wave w runs the 32-position tiles w, w + 4, ...; all-zero 16-k steps are skipped (the
//            accumulator never holds -0, so they change no bit).
//   between  the same LDS becomes the chunk's image [32][s R + 3 - s][LW] of the band (a channel's rows padded to 4
//            elements mod 128, so that the 32 channels of an epilogue store fall into different banks): zeroed first
//            -- the ring columns, and the ring row where the band touches the top (or, at stride 1, the bottom) of the
//            plane -- then filled with the real rows, the neighbour bands' rows included.  Image column j sits at
//            index j + 8.
//   phase 2  per output dw_finish's arithmetic (accumulator from 0.0f, nine fmaf with ky outer and kx inner, acc +
//            bias, activate, settled(), one rounding through K11's element types), no bounds test.  NOT the generic
//            kernel's walk: 8, 16, ... 256 threads per channel (256 / live channels), a thread owns segments of 8 (OW %
//            8 == 0) or 4 horizontally adjacent outputs, its window read from LDS, one 16- or 8-byte store each.
//
// The workgroups of one image run on one XCD, the chunks of a band next to each other, so x is re-read out of that
// XCD's L2.  No atomics, no split-K, no workspace: the same inputs give the same bits.
#include "common.h"

namespace mtr {

typedef float edt_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short edt_u16x8 __attribute__((ext_vector_type(8)));

template <int DT> struct EdtBits;
template <> struct EdtBits<MTR_F16> {
  typedef __half T;  // K11's element type: phase 2 rounds and widens exactly as depthwise.hip does
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
  static __device__ __forceinline__ edt_f32x16 mfma(uint4 a, uint4 b, edt_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};
template <> struct EdtBits<MTR_BF16> {
  typedef __hip_bfloat16 T;
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
  static __device__ __forceinline__ edt_f32x16 mfma(uint4 a, uint4 b, edt_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};

constexpr int kEdtBK = 32;       // k-tile of the X^T image
constexpr int kEdtCM = 32;       // expanded channels per workgroup
constexpr int kEdtColPad = 8;    // image column j of the chunk's image sits at index j + 8
constexpr size_t kEdtMaxLds = 160 * 1024;
constexpr size_t kEdtLdsTarget = 80 * 1024;  // what the band height is chosen for: two workgroups per CU

struct EdtGeo {
  int Cin, Cmid, H, W, HW, OH, OW;
  int R;                 // output rows per band
  int rows_img;          // rows of the chunk's image = input rows of a band: s R + 3 - s
  int LW, plane;         // elements per row and per channel (rows_img LW padded to 4 mod 128) of the chunk's image
  int ldk;               // elements per position of the X^T image: min(32, Cin rounded up to 16) + 8
  int chunks, bands;     // workgroups per image = chunks * bands
  int sw8;               // 1: segments of 8 outputs (OW % 8 == 0), 0: of 4
  int ns;                // segments per output row
  FastDiv d_w, d_ns, d_chunks, d_wgs;  // by W, ns, chunks, chunks * bands
};

// FN 32-position tiles per wave, four waves along the positions: BN = 128 FN staged positions per band
template <int DT, int S, int FN>
__global__ __launch_bounds__(256) void expand_dw16_tiles_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w1, const float* __restrict__ bias1,
    const float* __restrict__ wd, const float* __restrict__ bias2, unsigned short* __restrict__ y, EdtGeo g, int B,
    int act1, int act2) {
  using Hh = EdtBits<DT>;
  using T = typename Hh::T;
  constexpr int CM = kEdtCM, BN = 128 * FN, BK = kEdtBK, KS = BK / 16;
  constexpr int UNITS = (BK / 4) * (BN / 8);  // loader units of 4 k x 8 positions
  constexpr int NU = UNITS / 256;             // units per loader thread
  extern __shared__ __attribute__((aligned(16))) unsigned short edt_lds[];
  unsigned short* xs = edt_lds;  // phase 1: [BN][ldk], the X^T image of a k-tile
  unsigned short* ms = edt_lds;  // afterwards: [CM][rows_img][LW], the chunk's band of the expanded activation

  // the workgroups of one image on one XCD (blockIdx.x % 8), band by band, the chunks of a band adjacent
  const int q = (int)blockIdx.x >> 3;
  const int qi = (int)fastdiv((unsigned)q, g.d_wgs);
  const int b = qi * 8 + ((int)blockIdx.x & 7);
  if (b >= B) return;  // (the whole workgroup, before any barrier)
  const int within = q - qi * (g.chunks * g.bands);
  const int band = (int)fastdiv((unsigned)within, g.d_chunks), chunk = within - band * g.chunks;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int M = g.Cmid, K = g.Cin, HW = g.HW;
  const int m0 = chunk * CM;
  // the band: output rows oy0 .. oy0 + R - 1, image row j = input row iy0 + j; the staged span of positions
  const int oy0 = band * g.R, iy0 = S * oy0 - 1;
  const int row_lo = iy0 < 0 ? 0 : iy0;
  const int row_hi = iy0 + g.rows_img < g.H ? iy0 + g.rows_img : g.H;
  const int p_lo = row_lo * g.W, p_hi = row_hi * g.W;
  const int p_base = p_lo & ~7;           // (H W % 8 == 0: whole 16-byte groups up to p_hi rounded up)
  const int n_pos = p_hi - p_base;        // <= BN (the host's choice of R)
  const int n_pos32 = (n_pos + 31) & ~31;
  const int ldk = g.ldk;

  // ---- phase 1: conv1x1_16_kernel's loop over the positions p_base .. p_hi - 1 of one image
  const unsigned short* xb = x + (long long)b * K * HW + p_base;
  edt_u16x8 xr[NU][4];
  auto load_x = [&](int k0) {
#pragma unroll
    for (int n = 0; n < NU; ++n) {
      const int u = tid + 256 * n;
      const int p8 = u % (BN / 8), k4 = u / (BN / 8);
      const bool on = 8 * p8 < n_pos;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = k0 + 4 * k4 + i;
        edt_u16x8 t = (edt_u16x8)0;
        if (on && k < K)
          t = __builtin_bit_cast(edt_u16x8, *reinterpret_cast<const uint4*>(xb + (long long)k * HW + 8 * p8));
        xr[n][i] = t;
      }
    }
  };
  auto store_x = [&]() {  // 4 k-rows x 8 positions -> 8 positions x 4 k of the X^T image
#pragma unroll
    for (int n = 0; n < NU; ++n) {
      const int u = tid + 256 * n;
      const int p8 = u % (BN / 8), k4 = u / (BN / 8);
      if (8 * p8 < n_pos32 && 4 * k4 + 8 < ldk) {  // (the tiles that run; the k columns the image has)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          uint2 v;
          v.x = (unsigned)xr[n][0][j] | ((unsigned)xr[n][1][j] << 16);
          v.y = (unsigned)xr[n][2][j] | ((unsigned)xr[n][3][j] << 16);
          *reinterpret_cast<uint2*>(&xs[(8 * p8 + j) * ldk + 4 * k4]) = v;
        }
      }
    }
  };
  // this lane's weight fragments: row m0 + r, k 16 s + 8 h .. + 7 of each k-tile
  const int mrow = m0 + r;
  auto load_w = [&](uint4 (&wr)[KS], int k0) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = k0 + 16 * s + 8 * h;
      uint4 t = make_uint4(0u, 0u, 0u, 0u);
      if (mrow < M && k < K) t = *reinterpret_cast<const uint4*>(w1 + (long long)mrow * K + k);
      wr[s] = t;
    }
  };

  edt_f32x16 acc[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;

  uint4 wc[KS], wnx[KS];
  const int n_tiles = (K + BK - 1) / BK;
  load_x(0);
  load_w(wc, 0);
  for (int t = 0; t < n_tiles; ++t) {
    store_x();
    __syncthreads();
    if (t + 1 < n_tiles) {  // in flight during this tile's MFMAs
      load_x((t + 1) * BK);
      load_w(wnx, (t + 1) * BK);
    }
    const unsigned short* xa = &xs[r * ldk + 8 * h];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (t * BK + 16 * s < K) {  // (uniform) a 16-k step past Cin adds +0 to an accumulator that is never -0
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int p0 = 32 * (4 * j + wave);
          if (p0 < n_pos) {  // (wave-uniform) tiles past the band do not run
            const uint4 a = *reinterpret_cast<const uint4*>(xa + p0 * ldk + 16 * s);
            acc[j] = Hh::mfma(a, wc[s], acc[j]);
          }
        }
      }
    }
    __syncthreads();  // the image is read: the next tile's, or the chunk's image, may overwrite it
    if (t + 1 < n_tiles) {
#pragma unroll
      for (int s = 0; s < KS; ++s) wc[s] = wnx[s];
    }
  }

  // ---- zero the chunk's image, ring included
  {
    const int n16 = (CM * g.plane) >> 3;  // (LW % 4 == 0, CM % 2 == 0: whole 16-byte groups)
    for (int i = tid; i < n16; i += 256) reinterpret_cast<uint4*>(ms)[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  // K13h's epilogue: the lane holds channel m0 + r, positions 8 q + 4 h + 0 .. 3 of each 32-position tile (inside one
  // row of the plane: W % 4 == 0, p_base % 4 == 0)
  auto epilogue = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
    if (m0 + r >= M) return;
    const float bm = bias1[m0 + r];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int p = p_base + 32 * (4 * j + wave) + 8 * qq + 4 * h;
        if (p < p_lo || p >= p_hi) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = settled(activate<ACT>(acc[j][4 * qq + e] + bm));
        uint2 o;
        o.x = (unsigned)Hh::rnd(v[0]) | ((unsigned)Hh::rnd(v[1]) << 16);
        o.y = (unsigned)Hh::rnd(v[2]) | ((unsigned)Hh::rnd(v[3]) << 16);
        const int row = (int)fastdiv((unsigned)p, g.d_w), col = p - row * g.W;
        *reinterpret_cast<uint2*>(&ms[r * g.plane + (row - iy0) * g.LW + kEdtColPad + col]) = o;
      }
    }
  };
  with_act(act1, epilogue);
  __syncthreads();

  // ---- phase 2: dw_finish's arithmetic per output, the taps from LDS (the ring is zero: no masks)
  const int live = M - m0 < CM ? M - m0 : CM;  // channels of this chunk
  int tpc_log2 = 3;                            // threads per channel: 8 .. 256
  while ((2 << tpc_log2) * live <= 256) ++tpc_log2;
  const int c = tid >> tpc_log2, sub = tid & ((1 << tpc_log2) - 1);
  auto depthwise = [&](auto tag, auto width) {
    constexpr int ACT = decltype(tag)::value;
    constexpr int SW = decltype(width)::value;  // outputs of a segment
    constexpr int NV = S * SW;                  // aligned elements of a window row; + the column left of them
    constexpr int NIN = S * (SW - 1) + 3;       // (stride 1: + the column right of them)
    struct alignas(SW * sizeof(T)) Seg { T v[SW]; };
    if (c >= live) return;
    const int m = m0 + c;
    float wk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = wd[m * 9 + k];
    const float bb = bias2[m];
    const unsigned short* mplane = ms + c * g.plane;
    unsigned short* yplane = y + ((size_t)b * (size_t)M + (size_t)m) * (size_t)(g.OH * g.OW);
    const int rows = oy0 + g.R <= g.OH ? g.R : g.OH - oy0;  // (a partial last band)
    const int n_seg = rows * g.ns;
    for (int it = sub; it < n_seg; it += 1 << tpc_log2) {
      const int oyl = (int)fastdiv((unsigned)it, g.d_ns), ox0 = (it - oyl * g.ns) * SW;
      // image rows S oyl .. + 2; columns S ox0 - 1 .. = indices kEdtColPad + S ox0 - 1 ..
      const unsigned short* mp = mplane + (S * oyl) * g.LW + kEdtColPad + S * ox0;
      float a[SW];
#pragma unroll
      for (int o = 0; o < SW; ++o) a[o] = 0.0f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const unsigned short* row = mp + ky * g.LW;
        float in[NIN];
        in[0] = to_f32(__builtin_bit_cast(T, row[-1]));
#pragma unroll
        for (int n = 0; n < NV / 4; ++n) {
          const uint2 raw = *reinterpret_cast<const uint2*>(row + 4 * n);
          in[1 + 4 * n] = to_f32(__builtin_bit_cast(T, (unsigned short)(raw.x & 0xffffu)));
          in[2 + 4 * n] = to_f32(__builtin_bit_cast(T, (unsigned short)(raw.x >> 16)));
          in[3 + 4 * n] = to_f32(__builtin_bit_cast(T, (unsigned short)(raw.y & 0xffffu)));
          in[4 + 4 * n] = to_f32(__builtin_bit_cast(T, (unsigned short)(raw.y >> 16)));
        }
        if constexpr (S == 1) in[NIN - 1] = to_f32(__builtin_bit_cast(T, row[NV]));
#pragma unroll
        for (int o = 0; o < SW; ++o)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) a[o] = fmaf(in[o * S + kx], wk[ky * 3 + kx], a[o]);
      }
      Seg out;
#pragma unroll
      for (int o = 0; o < SW; ++o) out.v[o] = T(settled(activate<ACT>(a[o] + bb)));
      *reinterpret_cast<Seg*>(yplane + (size_t)((oy0 + oyl) * g.OW + ox0)) = out;
    }
  };
  with_act(act2, [&](auto tag) {
    if (g.sw8) depthwise(tag, ActTag<8>());
    else depthwise(tag, ActTag<4>());
  });
}

static int edt_ilog2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

// launch_depthwise's condition for K11's stride-1 block kernel (depthwise.hip), restated for a 16-byte aligned x
static bool edt_k11_block_plane(int H, int W) {
  if (H % 4 || W % 4) return false;
  const int tw = edt_ilog2_exact(W / 4), th = edt_ilog2_exact(H / 4);
  return tw >= 0 && tw <= 4 && th >= 0 && tw + th <= 6;
}

// elements per channel of the image of `rows` rows: 4 (mod 128), two LDS banks from one channel to the next -- phase
// 1's epilogue writes one 8-byte group per channel (lane) at the same row and column
static int edt_plane(const EdtGeo& g, int rows) { return (rows * g.LW + 123) / 128 * 128 + 4; }

// the image of a band of R output rows: whether its staged span fits BN positions and its LDS the target
static bool edt_band_fits(const EdtGeo& g, int stride, int R, int BN) {
  const int rows = stride * R + 3 - stride;
  const int slack = g.W % 8 ? 4 : 0;  // the span starts at the 16-byte boundary at or below the first row
  return rows * g.W + slack <= BN && (size_t)kEdtCM * edt_plane(g, rows) * 2 <= kEdtLdsTarget;
}

// the shape rules of the entry (MTR_E_SHAPE: the caller keeps the two-kernel chain); fills g but for the band
static int expand_dw16_tiles_shape(EdtGeo& g, long long B, int Cin, int Cmid, int H, int W, int stride) {
  if (B < 0 || Cin <= 0 || Cmid <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (stride != 1 && stride != 2) return MTR_E_SHAPE;
  if (Cin % 8) return MTR_E_SHAPE;  // 16-byte groups of k
  if (H > 128 || W > 128) return MTR_E_SHAPE;
  if (stride == 1) {
    if (W % 4 || W < 4 || (H * W) % 8) return MTR_E_SHAPE;  // whole groups of four outputs, of eight positions
    if (edt_k11_block_plane(H, W)) return MTR_E_SHAPE;      // (K11's block kernel: other bits)
  } else {
    if (H % 2 || W % 8) return MTR_E_SHAPE;  // padding 1 on all four sides, OW % 4 == 0
  }
  if (B * Cmid >= (1LL << 30)) return MTR_E_SHAPE;  // (the generic kernel's own limit)
  if ((long long)Cin * H * W > 0x7fffffffLL || (long long)Cmid * 9 > 0x7fffffffLL) return MTR_E_SHAPE;
  g = EdtGeo{};
  g.Cin = Cin, g.Cmid = Cmid, g.H = H, g.W = W, g.HW = H * W;
  g.OH = stride == 1 ? H : H / 2, g.OW = stride == 1 ? W : W / 2;
  // column j at index j + 8; stride 1 reads one column right of the plane, rows stay whole 16-byte groups
  g.LW = stride == 1 ? (W + kEdtColPad + 1 + 7) / 8 * 8 : W + kEdtColPad;
  g.ldk = (Cin <= 16 ? 16 : kEdtBK) + 8;
  g.chunks = (Cmid + kEdtCM - 1) / kEdtCM;
  g.sw8 = g.OW % 8 == 0;
  g.ns = g.OW / (g.sw8 ? 8 : 4);
  g.d_w = make_fastdiv((unsigned)W);
  g.d_ns = make_fastdiv((unsigned)g.ns);
  g.d_chunks = make_fastdiv((unsigned)g.chunks);
  return MTR_OK;
}

struct EdtArgs {
  const void *x, *w1;
  const float *bias1, *wd, *bias2;
  void* y;
  int act1, act2;
  long long B;
  hipStream_t stream;
};

// y == NULL: the shape query (mtr_expand_dw16_tiles_lds_bytes), -> the bytes of LDS, no launch
template <int DT, int S, int FN>
static int launch_expand_dw16_tiles_cfg(const EdtArgs& a, EdtGeo g, int R) {
  constexpr int BN = 128 * FN;
  g.R = R;
  g.rows_img = S * R + 3 - S;
  g.plane = edt_plane(g, g.rows_img);
  g.bands = (g.OH + R - 1) / R;
  g.d_wgs = make_fastdiv((unsigned)(g.chunks * g.bands));
  const size_t xs_bytes = (size_t)BN * g.ldk * sizeof(unsigned short);
  const size_t ms_bytes = (size_t)kEdtCM * g.plane * sizeof(unsigned short);
  const size_t lds = xs_bytes > ms_bytes ? xs_bytes : ms_bytes;
  if (lds > kEdtMaxLds) return MTR_E_SHAPE;
  const long long gx = (a.B + 7) / 8 * 8 * g.chunks * g.bands;
  if (gx > 0x7fffffffLL) return MTR_E_SHAPE;
  if (!a.y) return (int)lds;
  auto kern = expand_dw16_tiles_kernel<DT, S, FN>;
  if (lds > 64 * 1024) {
    const int e = allow_dynamic_lds((const void*)kern, kEdtMaxLds);
    if (e != MTR_OK) return e;
  }
  MTR_CLEAR_STALE();
  hipLaunchKernelGGL(kern, dim3((unsigned)gx), dim3(256), lds, a.stream, (const unsigned short*)a.x,
                     (const unsigned short*)a.w1, a.bias1, a.wd, a.bias2, (unsigned short*)a.y, g, (int)a.B, a.act1,
                     a.act2);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

// the only place that maps a shape to the band height and the template parameters: the tallest band up to 8
// (stride 1) or 4 (stride 2) output rows whose input rows fit 512 staged positions; 1024 where that leaves fewer than
// 6 (3) rows -- rows of more than 64 (stride 2: 72) positions
template <int DT, int S>
static int launch_expand_dw16_tiles(const EdtArgs& a, const EdtGeo& g) {
  const int cap = S == 1 ? 8 : 4, want = S == 1 ? 6 : 3;
  auto tallest = [&](int BN) {
    int R = g.OH < cap ? g.OH : cap;
    while (R >= 1 && !edt_band_fits(g, S, R, BN)) --R;
    return R;
  };
  const int R4 = tallest(512);
  if (R4 >= (g.OH < want ? g.OH : want)) return launch_expand_dw16_tiles_cfg<DT, S, 4>(a, g, R4);
  const int R8 = tallest(1024);
  if (R8 < 1) return MTR_E_SHAPE;  // (no plane of the domain: three rows of 128 positions fit)
  return launch_expand_dw16_tiles_cfg<DT, S, 8>(a, g, R8);
}

template <int DT>
static int launch_expand_dw16_tiles_stride(const EdtArgs& a, const EdtGeo& g, int stride) {
  return stride == 1 ? launch_expand_dw16_tiles<DT, 1>(a, g) : launch_expand_dw16_tiles<DT, 2>(a, g);
}

}  // namespace mtr

extern "C" size_t mtr_expand_dw16_tiles_lds_bytes(long long B, int Cin, int Cmid, int H, int W, int stride) {
  mtr::EdtGeo g;
  if (B <= 0 || mtr::expand_dw16_tiles_shape(g, B, Cin, Cmid, H, W, stride) != MTR_OK) return 0;
  // (the tile and LDS rules do not depend on the dtype)
  mtr::EdtArgs a = {};
  a.B = B;
  const int n = mtr::launch_expand_dw16_tiles_stride<MTR_F16>(a, g, stride);
  return n > 0 ? (size_t)n : 0;
}

extern "C" int mtr_expand_dw16_tiles(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                                     const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin,
                                     int Cmid, int H, int W, int stride, void* y, mtr_stream_t stream) {
  if (!x || !w1 || !bias1 || !w_dw || !bias_dw || !y) return MTR_E_NULL;
  if (dtype != MTR_F16 && dtype != MTR_BF16) return MTR_E_DTYPE;
  mtr::EdtGeo g;
  const int e = mtr::expand_dw16_tiles_shape(g, B, Cin, Cmid, H, W, stride);
  if (e != MTR_OK) return e;
  if (act1_code < mtr::kActNone || act1_code > mtr::kActHardswish || act2_code < mtr::kActNone ||
      act2_code > mtr::kActHardswish)
    return MTR_E_PARAM;
  if (((uintptr_t)x % 16) || ((uintptr_t)w1 % 16) || ((uintptr_t)y % 16) || ((uintptr_t)bias1 % 4) ||
      ((uintptr_t)w_dw % 4) || ((uintptr_t)bias_dw % 4))
    return MTR_E_ALIGN;
  {  // y is written while other workgroups still read x
    const uintptr_t xb = (uintptr_t)x, yb = (uintptr_t)y;
    const uintptr_t xn = (uintptr_t)B * Cin * g.HW * 2, yn = (uintptr_t)B * Cmid * g.OH * g.OW * 2;
    if (x == y || (xb < yb + yn && yb < xb + xn)) return MTR_E_PARAM;
  }
  if (B == 0) return MTR_OK;
  const mtr::EdtArgs a = {x, w1, bias1, w_dw, bias_dw, y, act1_code, act2_code, B, (hipStream_t)stream};
  return dtype == MTR_F16 ? mtr::launch_expand_dw16_tiles_stride<MTR_F16>(a, g, stride)
                          : mtr::launch_expand_dw16_tiles_stride<MTR_BF16>(a, g, stride);
}
