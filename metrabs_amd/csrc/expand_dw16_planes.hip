// K26h: K25h's function (expand_dw16.hip: the 1x1 expand convolution of an MBConv block and the depthwise 3x3 stride-1
// convolution behind it, f16 / bf16, ONE launch, the expanded activation kept in LDS) on the planes K25h refuses
// because K11 runs them on its GENERIC kernel: 24x24 and 12x12 of the EfficientNetV2 family at 384 px, and every
// other plane up to 576 positions whose W / 4 or H / 4 is no power of two.
//
// Not part of the reference's hot path (like K10 - K25h): backbones.fold_batchnorm(dtype=f16 / bf16,
// fuse_expand_depthwise_planes=True).  Per image b, K25h's three formulas:
//
//   mid[b, c, p] = rnd16(act1(bias1[c] + sum_k W1[c, k] * x[b, k, p]))                                  c < Cmid
//   y[b, c, p]   = rnd16(act2(bias2[c] + sum_{ky, kx} Wd[c, ky, kx] * mid[b, c, p + (ky - 1, kx - 1)]))
//   mean[b, c]   = (1 / HW) * sum_p f32(y[b, c, p])                                                    (optional)
//
// with the BITS of conv1x1_16_kernel (K13h) followed by depthwise3x3_kernel (K11's generic kernel) -- which are also
// the bits of K13h + K18 (depthwise3x3_blocks.hip).  A workgroup of four waves owns CM expanded channels of one image
// over the whole plane:
//
//   phase 1  K13h's GEMM exactly as K25h runs it (16-k steps at k = 0, 16, ... on v_mfma_f32_32x32x16_{f16,bf16}, k
//            past Cin and positions past H W zero-filled, the X^T image in two LDS buffers in k-tiles of 32, the weight
//            fragments from global memory one k-tile ahead; bias + activation in f32, one plain-cast rounding behind
//            `settled`).  K13h's bits do not depend on the tile, so the plane is cut into ceil(H W / 32) position tiles
//            of any count: FN per wave, WN waves along the positions (the tiles past the plane compute zeros and store
//            nothing).  A loader thread owns up to three units of 4 k x 8 positions.
//   between  the same LDS becomes the slice's image [c][H + 2][W + 8] inside a zero ring (image column j at index
//            j + 4), zeroed first; the (row, column) of a position comes from a division by W.
//   phase 2  depthwise3x3_kernel's mapping and arithmetic: lpp = min(64, next power of two >= groups) lanes per
//            channel (groups = H W / 4 groups of four horizontally adjacent outputs), 64 / lpp channels per wave, lane
//            `sub` walks the groups sub, sub + 64, ...  Per output the accumulator starts at 0, nine fmaf with ky outer
//            and kx inner, acc + bias, activate, settled(), one rounding through K11's element types.  The mean: each
//            group summed left to right from 0.0f, the lane's groups added in ascending order from 0.0f, the xor
//            butterfly lpp / 2 .. 1, times 1.0f / (float)(H W).  No LDS for partial sums.
//
// The workgroup-to-image mapping is K25h's (by default the chunks of one image on one XCD; the bits do not depend on
// it).  No atomics, no split-K, no workspace: the same inputs give the same bits.
#include "common.h"

namespace mtr {

typedef float edp_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short edp_u16x8 __attribute__((ext_vector_type(8)));

template <int DT> struct EdpBits;
template <> struct EdpBits<MTR_F16> {
  typedef __half T;  // K11's element type: phase 2 rounds and widens exactly as depthwise.hip does
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
  static __device__ __forceinline__ edp_f32x16 mfma(uint4 a, uint4 b, edp_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};
template <> struct EdpBits<MTR_BF16> {
  typedef __hip_bfloat16 T;
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
  static __device__ __forceinline__ edp_f32x16 mfma(uint4 a, uint4 b, edp_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};

constexpr int kEdpBK = 32;               // k-tile of the X^T image
constexpr int kEdpLDK = kEdpBK + 8;      // its row (one position), padded like K13h's
constexpr int kEdpColPad = 4;            // image column j of the slice's image sits at index j + 4
constexpr size_t kEdpMaxLds = 160 * 1024;

struct EdpGeo {
  int Cin, Cmid, H, W, HW;
  int LW, plane;         // elements per row and per channel of the slice's image: W + 8, (H + 2) * LW
  int chunks;            // workgroups per image = ceil(Cmid / CM)
  int xcd_map;           // 1: the chunks of one image on one XCD
  int groups;            // groups of four outputs per plane = H * W / 4
  int lpp_log2;          // lanes per channel in phase 2 (depthwise3x3_kernel's lpp)
  int mchunks;           // groups a lane walks = ceil(groups / 64)
  float inv_hw;
  FastDiv d_w, d_w4;     // by W (phase 1's epilogue) and by W / 4 (phase 2's groups)
};

// The tiles of a workgroup of four waves: FN position tiles x one channel tile per wave, WN x WM waves,
// BN = 32 FN WN >= H W positions, CM = 32 WM channels per workgroup
//   up to  5 tiles (12x12, ...): FN 5, 1 x 4 waves, CM 128
//   up to 10 tiles (12x24, ...): FN 5, 2 x 2 waves, CM  64
//   up to 18 tiles (24x24, ...): FN 9, 2 x 2 waves, CM  64
template <int FN_, int WN_> struct EdpTiles {
  static constexpr int FN = FN_, WN = WN_, WM = 4 / WN_;
  static constexpr int CM = 32 * WM, BN = 32 * FN_ * WN_;
};

template <int DT, int FN, int WN>
__global__ __launch_bounds__(256) void expand_dw16_planes_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w1, const float* __restrict__ bias1,
    const float* __restrict__ wd, const float* __restrict__ bias2, unsigned short* __restrict__ y,
    float* __restrict__ row_mean, EdpGeo g, int B, int act1, int act2) {
  using Hh = EdpBits<DT>;
  using T = typename Hh::T;
  using Tl = EdpTiles<FN, WN>;
  constexpr int WM = Tl::WM, CM = Tl::CM, BN = Tl::BN;
  constexpr int BK = kEdpBK, LDK = kEdpLDK, KS = BK / 16;
  constexpr int UNITS = (BK / 4) * (BN / 8);  // loader units of 4 k x 8 positions
  constexpr int NU = (UNITS + 255) / 256;     // units per loader thread
  extern __shared__ __attribute__((aligned(16))) unsigned short edp_lds[];
  unsigned short* xs = edp_lds;  // phase 1: [2][BN * LDK], the X^T image of a k-tile
  unsigned short* ms = edp_lds;  // afterwards: [CM][H + 2][LW], the slice of the expanded activation

  int b, chunk;
  if (g.xcd_map) {
    const int q = (int)blockIdx.x >> 3;
    b = (q / g.chunks) * 8 + ((int)blockIdx.x & 7);
    chunk = q % g.chunks;
    if (b >= B) return;  // (the whole workgroup, before any barrier)
  } else {
    b = (int)blockIdx.x / g.chunks;
    chunk = (int)blockIdx.x % g.chunks;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int r = lane & 31, h = lane >> 5;
  const int M = g.Cmid, K = g.Cin, HW = g.HW;
  const int m0 = chunk * CM;

  // ---- phase 1: conv1x1_16_kernel's loop over one image, columns 0 .. HW - 1 (past HW: zero-filled, never written)
  const unsigned short* xb = x + (long long)b * K * HW;
  edp_u16x8 xr[NU][4];
  auto load_x = [&](int k0) {
#pragma unroll
    for (int n = 0; n < NU; ++n) {
      const int u = tid + 256 * n;
      const int p8 = u % (BN / 8), k4 = u / (BN / 8);
      const bool on = u < UNITS && 8 * p8 < HW;  // (H W % 8 == 0: a unit is inside the plane or past it)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = k0 + 4 * k4 + i;
        edp_u16x8 t = (edp_u16x8)0;
        if (on && k < K)
          t = __builtin_bit_cast(edp_u16x8, *reinterpret_cast<const uint4*>(xb + (long long)k * HW + 8 * p8));
        xr[n][i] = t;
      }
    }
  };
  auto store_x = [&](int buf) {  // 4 k-rows x 8 positions -> 8 positions x 4 k of the X^T image
#pragma unroll
    for (int n = 0; n < NU; ++n) {
      const int u = tid + 256 * n;
      const int p8 = u % (BN / 8), k4 = u / (BN / 8);
      if (u < UNITS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          uint2 v;
          v.x = (unsigned)xr[n][0][j] | ((unsigned)xr[n][1][j] << 16);
          v.y = (unsigned)xr[n][2][j] | ((unsigned)xr[n][3][j] << 16);
          *reinterpret_cast<uint2*>(&xs[buf * (BN * LDK) + (8 * p8 + j) * LDK + 4 * k4]) = v;
        }
      }
    }
  };
  // this lane's weight fragments: row m0 + 32 wm + r, k 16 s + 8 h .. + 7 of each k-tile
  const int mrow = m0 + wm * 32 + r;
  auto load_w = [&](uint4 (&wr)[KS], int k0) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = k0 + 16 * s + 8 * h;
      uint4 t = make_uint4(0u, 0u, 0u, 0u);
      if (mrow < M && k < K) t = *reinterpret_cast<const uint4*>(w1 + (long long)mrow * K + k);
      wr[s] = t;
    }
  };

  edp_f32x16 acc[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;

  uint4 wc[KS], wnx[KS];
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
    const unsigned short* xa = &xs[buf * (BN * LDK) + (wn * (32 * FN) + r) * LDK + 8 * h];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const uint4 a = *reinterpret_cast<const uint4*>(xa + (32 * j) * LDK + 16 * s);
        acc[j] = Hh::mfma(a, wc[s], acc[j]);
      }
    }
    if (t + 1 < n_tiles) {
      store_x(buf ^ 1);  // the other buffer: last read before the previous barrier
#pragma unroll
      for (int s = 0; s < KS; ++s) wc[s] = wnx[s];
    }
    __syncthreads();
  }

  // ---- the X^T buffers are free (the barrier above): zero the slice's image, ring and dead channels included
  {
    const int n16 = (CM * g.plane) >> 3;  // (CM % 64 == 0, LW % 4 == 0: whole 16-byte groups)
    for (int i = tid; i < n16; i += 256) reinterpret_cast<uint4*>(ms)[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  // K13h's epilogue: the lane holds channel .. + r, positions 8 q + 4 h + 0 .. 3 of each 32-position tile (one row of
  // the plane: W % 4 == 0)
  auto epilogue = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
    const int cl = wm * 32 + r;
    if (m0 + cl >= M) return;
    const float bm = bias1[m0 + cl];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = wn * (32 * FN) + 32 * j + 8 * q + 4 * h;
        if (p >= HW) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = settled(activate<ACT>(acc[j][4 * q + e] + bm));
        uint2 o;
        o.x = (unsigned)Hh::rnd(v[0]) | ((unsigned)Hh::rnd(v[1]) << 16);
        o.y = (unsigned)Hh::rnd(v[2]) | ((unsigned)Hh::rnd(v[3]) << 16);
        const int row = (int)fastdiv((unsigned)p, g.d_w), col = p - row * g.W;
        *reinterpret_cast<uint2*>(&ms[cl * g.plane + (row + 1) * g.LW + kEdpColPad + col]) = o;
      }
    }
  };
  with_act(act1, epilogue);
  __syncthreads();

  // ---- phase 2: depthwise3x3_kernel's lanes and arithmetic, the taps from LDS (the ring is zero: no masks)
  const int lpp = 1 << g.lpp_log2, ppi = 64 >> g.lpp_log2;
  const int sub = lane & (lpp - 1), pl = lane >> g.lpp_log2;
  const int w4 = g.W >> 2;
  auto depthwise = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
    struct alignas(4 * sizeof(T)) V4 { T v[4]; };
    // (CM is a multiple of 4 ppi wherever ppi > 1 -- those planes run CM = 128 -- so c < CM for every lane)
    for (int c0 = wave * ppi; c0 < CM; c0 += 4 * ppi) {
      if (m0 + c0 >= M) break;  // (wave-uniform: the wave's first channel is past Cmid, and so are all later ones)
      const int c = c0 + pl, m = m0 + c;
      const bool live = m < M;
      const int mc = live ? m : M - 1;  // dead lanes: zeros from LDS, the last channel's weights, no store
      float wk[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) wk[k] = wd[mc * 9 + k];
      const float bb = bias2[mc];
      const unsigned short* mplane = ms + c * g.plane;
      unsigned short* yplane = y + ((size_t)b * (size_t)M + (size_t)mc) * (size_t)HW;
      float sum = 0.0f;
      for (int ch = 0; ch < g.mchunks; ++ch) {
        const int v0 = ch * 64 + sub;
        const bool on = live && v0 < g.groups;
        const int v = v0 < g.groups ? v0 : g.groups - 1;
        const int oy = (int)fastdiv((unsigned)v, g.d_w4), ox0 = (v - oy * w4) << 2;
        // rows oy - 1 .. oy + 1 of the plane = rows oy .. oy + 2 of the image; columns ox0 - 1 .. ox0 + 4 = indices
        // ox0 + 3 .. ox0 + 8
        const unsigned short* mp = mplane + oy * g.LW + ox0;
        float a4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const unsigned short* row = mp + ky * g.LW;
          const V4 mid4 = *reinterpret_cast<const V4*>(row + kEdpColPad);
          float in[6];
          in[0] = to_f32(__builtin_bit_cast(T, row[kEdpColPad - 1]));
#pragma unroll
          for (int j = 0; j < 4; ++j) in[1 + j] = to_f32(mid4.v[j]);
          in[5] = to_f32(__builtin_bit_cast(T, row[kEdpColPad + 4]));
#pragma unroll
          for (int o = 0; o < 4; ++o)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) a4[o] = fmaf(in[o + kx], wk[ky * 3 + kx], a4[o]);
        }
        V4 out;
        float s = 0.0f;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const float a = settled(activate<ACT>(a4[o] + bb));
          out.v[o] = T(a);
          s += to_f32(out.v[o]);
        }
        if (on) *reinterpret_cast<V4*>(yplane + oy * g.W + ox0) = out;
        sum += on ? s : 0.0f;
      }
      if (row_mean) {
        for (int mk = lpp >> 1; mk >= 1; mk >>= 1) sum += __shfl_xor(sum, mk, 64);
        if (live && sub == 0) row_mean[(size_t)b * (size_t)M + (size_t)m] = sum * g.inv_hw;
      }
    }
  };
  with_act(act2, depthwise);
}

static int edp_ilog2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

// launch_depthwise's condition for K11's stride-1 block kernel (depthwise.hip), restated for a 16-byte aligned x
static bool edp_k11_block_plane(int H, int W) {
  if (H % 4 || W % 4) return false;
  const int tw = edp_ilog2_exact(W / 4), th = edp_ilog2_exact(H / 4);
  return tw >= 0 && tw <= 4 && th >= 0 && tw + th <= 6;
}

// the shape rules of the entry (MTR_E_SHAPE: the caller keeps the two-kernel chain); fills g
static int expand_dw16_planes_shape(EdpGeo& g, long long B, int Cin, int Cmid, int H, int W) {
  if (B < 0 || Cin <= 0 || Cmid <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (Cin % 8 || W % 4) return MTR_E_SHAPE;  // 16-byte groups of k; whole groups of four outputs
  if (H > 32 || W > 32 || H * W > 576 || (H * W) % 8) return MTR_E_SHAPE;  // 16-byte groups of positions
  if (edp_k11_block_plane(H, W)) return MTR_E_SHAPE;  // (K11's block kernel: other bits; K25h's planes among them)
  if (B * Cmid >= (1LL << 30)) return MTR_E_SHAPE;  // (the generic kernel's own limit)
  const int HW = H * W;
  if ((long long)Cin * HW > 0x7fffffffLL || (long long)Cmid * 9 > 0x7fffffffLL) return MTR_E_SHAPE;
  g = EdpGeo{};
  g.Cin = Cin, g.Cmid = Cmid, g.H = H, g.W = W, g.HW = HW;
  g.LW = W + 2 * kEdpColPad, g.plane = (H + 2) * g.LW;
  g.xcd_map = 1;
  g.groups = HW / 4;
  g.lpp_log2 = 0;
  while ((1 << g.lpp_log2) < 64 && (1 << g.lpp_log2) < g.groups) ++g.lpp_log2;
  g.mchunks = (g.groups + 63) / 64;
  g.inv_hw = 1.0f / (float)(H * W);
  g.d_w = make_fastdiv((unsigned)W);
  g.d_w4 = make_fastdiv((unsigned)(W / 4));
  return MTR_OK;
}

struct EdpArgs {
  const void *x, *w1;
  const float *bias1, *wd, *bias2;
  void* y;
  float* row_mean;
  int act1, act2;
  long long B;
  hipStream_t stream;
};

// y == NULL: the shape query (mtr_expand_dw16_planes_lds_bytes), -> the bytes of LDS, no launch
template <int DT, int FN, int WN>
static int launch_expand_dw16_planes_cfg(const EdpArgs& a, EdpGeo g) {
  using Tl = EdpTiles<FN, WN>;
  g.chunks = (g.Cmid + Tl::CM - 1) / Tl::CM;
  const size_t xs_bytes = (size_t)2 * Tl::BN * kEdpLDK * sizeof(unsigned short);
  const size_t ms_bytes = (size_t)Tl::CM * g.plane * sizeof(unsigned short);
  const size_t lds = xs_bytes > ms_bytes ? xs_bytes : ms_bytes;
  if (lds > kEdpMaxLds) return MTR_E_SHAPE;
  const long long images = g.xcd_map ? (a.B + 7) / 8 * 8 : a.B;
  const long long gx = images * g.chunks;
  if (gx > 0x7fffffffLL) return MTR_E_SHAPE;
  if (!a.y) return (int)lds;
  auto kern = expand_dw16_planes_kernel<DT, FN, WN>;
  if (lds > 64 * 1024) {
    const int e = allow_dynamic_lds((const void*)kern, kEdpMaxLds);
    if (e != MTR_OK) return e;
  }
  MTR_CLEAR_STALE();
  hipLaunchKernelGGL(kern, dim3((unsigned)gx), dim3(256), lds, a.stream, (const unsigned short*)a.x,
                     (const unsigned short*)a.w1, a.bias1, a.wd, a.bias2, (unsigned short*)a.y, a.row_mean, g,
                     (int)a.B, a.act1, a.act2);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

// the only place that maps a plane to template parameters
template <int DT>
static int launch_expand_dw16_planes(const EdpArgs& a, const EdpGeo& g) {
  const int npt = (g.HW + 31) / 32;
  if (npt <= 5) return launch_expand_dw16_planes_cfg<DT, 5, 1>(a, g);
  if (npt <= 10) return launch_expand_dw16_planes_cfg<DT, 5, 2>(a, g);
  return launch_expand_dw16_planes_cfg<DT, 9, 2>(a, g);
}

}  // namespace mtr

extern "C" size_t mtr_expand_dw16_planes_lds_bytes(long long B, int Cin, int Cmid, int H, int W) {
  mtr::EdpGeo g;
  if (B <= 0 || mtr::expand_dw16_planes_shape(g, B, Cin, Cmid, H, W) != MTR_OK) return 0;
  // (the tile and LDS rules do not depend on the dtype)
  mtr::EdpArgs a = {};
  a.B = B;
  const int n = mtr::launch_expand_dw16_planes<MTR_F16>(a, g);
  return n > 0 ? (size_t)n : 0;
}

extern "C" int mtr_expand_dw16_planes_opts(const void* x, int dtype, const void* w1, const float* bias1,
                                           int act1_code, const float* w_dw, const float* bias_dw, int act2_code,
                                           long long B, int Cin, int Cmid, int H, int W, void* y, float* row_mean,
                                           mtr_stream_t stream, int mapping) {
  if (!x || !w1 || !bias1 || !w_dw || !bias_dw || !y) return MTR_E_NULL;
  if (dtype != MTR_F16 && dtype != MTR_BF16) return MTR_E_DTYPE;
  mtr::EdpGeo g;
  const int e = mtr::expand_dw16_planes_shape(g, B, Cin, Cmid, H, W);
  if (e != MTR_OK) return e;
  if (act1_code < mtr::kActNone || act1_code > mtr::kActHardswish || act2_code < mtr::kActNone ||
      act2_code > mtr::kActHardswish)
    return MTR_E_PARAM;
  if (mapping < -1 || mapping > 1) return MTR_E_PARAM;
  if (((uintptr_t)x % 16) || ((uintptr_t)w1 % 16) || ((uintptr_t)y % 16) || ((uintptr_t)bias1 % 4) ||
      ((uintptr_t)w_dw % 4) || ((uintptr_t)bias_dw % 4) || ((uintptr_t)row_mean % 4))
    return MTR_E_ALIGN;
  {  // y is written while other workgroups still read x
    const uintptr_t xb = (uintptr_t)x, yb = (uintptr_t)y;
    const uintptr_t xn = (uintptr_t)B * Cin * g.HW * 2, yn = (uintptr_t)B * Cmid * g.HW * 2;
    if (x == y || (xb < yb + yn && yb < xb + xn)) return MTR_E_PARAM;
  }
  if (B == 0) return MTR_OK;
  if (mapping >= 0) g.xcd_map = mapping;
  const mtr::EdpArgs a = {x, w1, bias1, w_dw, bias_dw, y, row_mean, act1_code, act2_code, B, (hipStream_t)stream};
  const int rc = dtype == MTR_F16 ? mtr::launch_expand_dw16_planes<MTR_F16>(a, g)
                                  : mtr::launch_expand_dw16_planes<MTR_BF16>(a, g);
  return rc;
}

extern "C" int mtr_expand_dw16_planes(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                                      const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin,
                                      int Cmid, int H, int W, void* y, float* row_mean, mtr_stream_t stream) {
  return mtr_expand_dw16_planes_opts(x, dtype, w1, bias1, act1_code, w_dw, bias_dw, act2_code, B, Cin, Cmid, H, W, y,
                                     row_mean, stream, -1);
}
