// K25h: the 1x1 expand convolution of an MBConv block (K13h, conv1x1_16.hip) and the depthwise 3x3 stride-1
// convolution behind it (K11's stride-1 block kernel, depthwise.hip) of f16 / bf16 tensors as ONE launch.  The
// expanded activation -- the widest tensor of the block, written once and read once by the chain -- stays in LDS.
//
// Not part of the reference's hot path (like K10 - K16h): the stride-1 MBConv blocks of the backbone's 16-bit
// inference copy (backbones.fold_batchnorm(dtype=f16 / bf16, fuse_expand_depthwise=True)).  Per image b:
//
//   mid[b, c, p] = rnd16(act1(bias1[c] + sum_k W1[c, k] * x[b, k, p]))                                  c < Cmid
//   y[b, c, p]   = rnd16(act2(bias2[c] + sum_{ky, kx} Wd[c, ky, kx] * mid[b, c, p + (ky - 1, kx - 1)]))
//   mean[b, c]   = (1 / HW) * sum_p f32(y[b, c, p])                                                    (optional)
//
// with the BITS of the two-kernel chain.  A depthwise convolution is per channel, so a workgroup that owns a slice of
// CM expanded channels of one image over the WHOLE plane (H W <= 256) needs nothing from another workgroup:
//
//   phase 1  K13h's GEMM for the slice, Y^T = X^T W^T on v_mfma_f32_32x32x16_{f16,bf16}: the same 16-k steps at
//            k = 0, 16, 32, ..., lane (r, h) holding the 8-k group 2 step + h, k past Cin zero-filled, the X^T image
//            staged through two LDS buffers in k-tiles of 32 exactly as conv1x1_16_kernel stages it, the weight
//            fragments as 16-byte loads from global memory one k-tile ahead.  Bias, activation (f32) and ONE
//            plain-cast rounding in registers; `settled` keeps the activation's last product an f32 value of its own,
//            as K13h's stored output is.
//   between  the X^T buffers are dead: the same LDS becomes the slice's image [c][H + 2][W + 8] (image column j at
//            index j + 4: 8-byte stores and loads), zeroed first, so the ring around every plane and the channels past
//            Cmid are zero and phase 2 needs no bounds test.
//   phase 2  one lane per (channel, 4 x 4 block of outputs), lanes indexed local = (ty << tw_log2) | tx inside an
//            aligned group of lp = H W / 16 lanes as in depthwise3x3_s1_block_kernel: the 6 x 6 window from LDS, the
//            accumulator started at the bias, nine fmaf in (ky, kx) order, settled(activate()), one rounding, four
//            8-byte row stores; the mean from the 16 rounded outputs in (row, column) order, the lp lanes combined by
//            __shfl_xor with m = lp / 2 .. 1, times 1.0f / (H * W).
//
// Every workgroup of an image re-reads that image's x (Cin HW 2 bytes) from L2.  Workgroups are dealt round-robin
// over the 8 XCDs, so by default the image index comes from blockIdx.x % 8 and blockIdx.x / (8 chunks): the chunks of
// one image land on one XCD and x crosses to one L2 (`mapping` 0 keeps blockIdx.x = image * chunks + chunk; the bits
// do not depend on it).  No atomics, no split-K, no workspace: the same inputs give the same bits.
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
constexpr int kEdwLDK = kEdwBK + 8;      // its row (one position), padded like K13h's
constexpr int kEdwColPad = 4;            // image column j of the slice's image sits at index j + 4
constexpr size_t kEdwMaxLds = 160 * 1024;

struct EdwGeo {
  int Cin, Cmid, H, W, HW;
  int tw_log2, lp_log2;  // blocks per row, lanes (4 x 4 blocks) per plane, as K11's block kernel counts them
  int LW, plane;         // elements per row and per channel of the slice's image: W + 8, (H + 2) * LW
  int chunks;            // workgroups per image = ceil(Cmid / CM)
  int xcd_map;           // 1: the chunks of one image on one XCD
  float inv_hw;
};

// The tiles of a workgroup of four waves, from NPT = the 32-position tiles of a plane (1, 2, 4, 8):
//   FN position tiles x FM channel tiles per wave, WN x WM waves, CM = 32 FM WM channels per workgroup
//   NPT 8 (16x16, ...): 4 x 1 per wave, 2 x 2 waves, CM  64     NPT 2 (8x8, ...): 2 x 1, 1 x 4, CM 128
//   NPT 4 (8x16, ...) : 4 x 1,          1 x 4,       CM 128     NPT 1 (4x4, 4x8): 1 x 2, 1 x 4, CM 256
template <int NPT> struct EdwTiles {
  static constexpr int FN = NPT < 4 ? NPT : 4, FM = NPT == 1 ? 2 : 1;
  static constexpr int WN = NPT / FN, WM = 4 / WN;
  static constexpr int CM = 32 * FM * WM, BN = 32 * NPT;
};

template <int DT, int NPT>
__global__ __launch_bounds__(256) void expand_dw16_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w1, const float* __restrict__ bias1,
    const float* __restrict__ wd, const float* __restrict__ bias2, unsigned short* __restrict__ y,
    float* __restrict__ row_mean, EdwGeo g, int B, int act1, int act2) {
  using Hh = EdwBits<DT>;
  using T = typename Hh::T;
  using Tl = EdwTiles<NPT>;
  constexpr int FN = Tl::FN, FM = Tl::FM, WM = Tl::WM, CM = Tl::CM, BN = Tl::BN;
  constexpr int BK = kEdwBK, LDK = kEdwLDK, KS = BK / 16;
  constexpr int UNITS = (BK / 4) * (BN / 8);  // loader units of 4 k x 8 positions
  static_assert(UNITS <= 256, "one loader unit per thread at most");
  extern __shared__ __attribute__((aligned(16))) unsigned short edw_lds[];
  unsigned short* xs = edw_lds;  // phase 1: [2][BN * LDK], the X^T image of a k-tile
  unsigned short* ms = edw_lds;  // afterwards: [CM][H + 2][LW], the slice of the expanded activation

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
  const int p8 = tid % (BN / 8), k4 = tid / (BN / 8);
  const bool xload = tid < UNITS && 8 * p8 < HW;
  const unsigned short* xsrc = x + (long long)b * K * HW + 8 * p8;
  edw_u16x8 xr[4];
  auto load_x = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + 4 * k4 + i;
      edw_u16x8 t = (edw_u16x8)0;
      if (xload && k < K) t = __builtin_bit_cast(edw_u16x8, *reinterpret_cast<const uint4*>(xsrc + (long long)k * HW));
      xr[i] = t;
    }
  };
  auto store_x = [&](int buf) {  // 4 k-rows x 8 positions -> 8 positions x 4 k of the X^T image
    if (tid < UNITS) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        uint2 v;
        v.x = (unsigned)xr[0][j] | ((unsigned)xr[1][j] << 16);
        v.y = (unsigned)xr[2][j] | ((unsigned)xr[3][j] << 16);
        *reinterpret_cast<uint2*>(&xs[buf * (BN * LDK) + (8 * p8 + j) * LDK + 4 * k4]) = v;
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
        if (m < M && k < K) t = *reinterpret_cast<const uint4*>(w1 + (long long)m * K + k);
        wr[i][s] = t;
      }
    }
  };

  edw_f32x16 acc[FM][FN];
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
    const unsigned short* xa = &xs[buf * (BN * LDK) + (wn * (32 * FN) + r) * LDK + 8 * h];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      uint4 a[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) a[j] = *reinterpret_cast<const uint4*>(xa + (32 * j) * LDK + 16 * s);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = Hh::mfma(a[j], wc[i][s], acc[i][j]);
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

  // ---- the X^T buffers are free (the barrier above): zero the slice's image, ring and dead channels included
  {
    const int n16 = (CM * g.plane) >> 3;  // (CM % 64 == 0, LW % 4 == 0: whole 16-byte groups)
    for (int i = tid; i < n16; i += 256) reinterpret_cast<uint4*>(ms)[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();
  // K13h's epilogue: the lane holds channel .. + r, positions 8 q + 4 h + 0 .. 3 of each 32-position tile (one row of
  // the plane: W % 4 == 0)
  const int w_log2 = g.tw_log2 + 2;
  auto epilogue = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int cl = wm * (32 * FM) + 32 * i + r;
      if (m0 + cl >= M) continue;
      const float bm = bias1[m0 + cl];
#pragma unroll
      for (int j = 0; j < FN; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int p = wn * (32 * FN) + 32 * j + 8 * q + 4 * h;
          if (p >= HW) continue;
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = settled(activate<ACT>(acc[i][j][4 * q + e] + bm));
          uint2 o;
          o.x = (unsigned)Hh::rnd(v[0]) | ((unsigned)Hh::rnd(v[1]) << 16);
          o.y = (unsigned)Hh::rnd(v[2]) | ((unsigned)Hh::rnd(v[3]) << 16);
          const int row = p >> w_log2, col = p & (g.W - 1);
          *reinterpret_cast<uint2*>(&ms[cl * g.plane + (row + 1) * g.LW + kEdwColPad + col]) = o;
        }
      }
    }
  };
  with_act(act1, epilogue);
  __syncthreads();

  // ---- phase 2: depthwise3x3_s1_block_kernel's arithmetic, the window from LDS instead of global memory and DPP
  const int lp_log2 = g.lp_log2, tw_log2 = g.tw_log2;
  const int local = tid & ((1 << lp_log2) - 1);
  const int ty = local >> tw_log2, tx = local & ((1 << tw_log2) - 1);
  const int oy0 = ty << 2, ox0 = tx << 2;
  auto depthwise = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
    struct alignas(4 * sizeof(T)) V4 { T v[4]; };
    for (int c = tid >> lp_log2; c < CM; c += 256 >> lp_log2) {  // (CM is a multiple of the step: every lane stays in)
      if (m0 + c - (lane >> lp_log2) >= M) continue;  // (wave-uniform: the wave's first channel is past Cmid)
      const int m = m0 + c;
      const bool live = m < M;
      const int mc = live ? m : M - 1;  // dead lanes: zeros from LDS, the last channel's weights, no store
      float wk[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) wk[k] = wd[mc * 9 + k];
      const float bb = bias2[mc];
      // rows oy0 - 1 .. oy0 + 4 of the plane = rows oy0 .. oy0 + 5 of the image; columns ox0 - 1 .. ox0 + 4 =
      // indices ox0 + 3 .. ox0 + 8
      const unsigned short* mp = ms + c * g.plane + oy0 * g.LW + ox0;
      float in[6][6];
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) {
        const unsigned short* row = mp + rr * g.LW;
        struct alignas(4 * sizeof(T)) R4 { T v[4]; };
        const R4 mid4 = *reinterpret_cast<const R4*>(row + kEdwColPad);
        in[rr][0] = to_f32(__builtin_bit_cast(T, row[kEdwColPad - 1]));
#pragma unroll
        for (int j = 0; j < 4; ++j) in[rr][1 + j] = to_f32(mid4.v[j]);
        in[rr][5] = to_f32(__builtin_bit_cast(T, row[kEdwColPad + 4]));
      }
      float sum = 0.0f;
      unsigned short* yp = y + ((size_t)b * (size_t)M + (size_t)mc) * (size_t)HW + oy0 * g.W + ox0;
#pragma unroll
      for (int orow = 0; orow < 4; ++orow) {
        float a4[4] = {bb, bb, bb, bb};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx)
#pragma unroll
            for (int o = 0; o < 4; ++o) a4[o] = fmaf(in[orow + ky][o + kx], wk[ky * 3 + kx], a4[o]);
        V4 out;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const float a = settled(activate<ACT>(a4[o]));
          out.v[o] = T(a);
          sum += to_f32(out.v[o]);
        }
        if (live) *reinterpret_cast<V4*>(yp + orow * g.W) = out;
      }
      if (row_mean) {
        for (int mk = (1 << lp_log2) >> 1; mk >= 1; mk >>= 1) sum += __shfl_xor(sum, mk, 64);
        if (live && local == 0) row_mean[(size_t)b * (size_t)M + (size_t)m] = sum * g.inv_hw;
      }
    }
  };
  with_act(act2, depthwise);
}

static int edw_ilog2_exact(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

// the shape rules of the entry (MTR_E_SHAPE: the caller keeps the two-kernel chain); fills g
static int expand_dw16_shape(EdwGeo& g, long long B, int Cin, int Cmid, int H, int W) {
  if (B < 0 || Cin <= 0 || Cmid <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (Cin % 8 || H % 4 || W % 4) return MTR_E_SHAPE;  // 16-byte groups of k; whole 4 x 4 blocks
  // the planes K11 runs on its stride-1 block kernel (launch_depthwise in depthwise.hip), up to 256 positions
  const int tw = edw_ilog2_exact(W / 4), th = edw_ilog2_exact(H / 4);
  if (tw < 0 || th < 0 || tw + th > 4) return MTR_E_SHAPE;
  if (B * Cmid >= (1LL << 24)) return MTR_E_SHAPE;  // (past this K11 takes its generic kernel: other bits)
  const int HW = H * W;
  if ((long long)Cin * HW > 0x7fffffffLL || (long long)Cmid * 9 > 0x7fffffffLL) return MTR_E_SHAPE;
  g = EdwGeo{};
  g.Cin = Cin, g.Cmid = Cmid, g.H = H, g.W = W, g.HW = HW;
  g.tw_log2 = tw, g.lp_log2 = tw + th;
  g.LW = W + 2 * kEdwColPad, g.plane = (H + 2) * g.LW;
  g.xcd_map = 1;
  g.inv_hw = 1.0f / (float)(H * W);
  return MTR_OK;
}

struct EdwArgs {
  const void *x, *w1;
  const float *bias1, *wd, *bias2;
  void* y;
  float* row_mean;
  int act1, act2;
  long long B;
  hipStream_t stream;
};

// y == NULL: the shape query (mtr_expand_dw16_lds_bytes), -> the bytes of LDS, no launch
template <int DT, int NPT>
static int launch_expand_dw16_cfg(const EdwArgs& a, EdwGeo g) {
  using Tl = EdwTiles<NPT>;
  g.chunks = (g.Cmid + Tl::CM - 1) / Tl::CM;
  const size_t xs_bytes = (size_t)2 * Tl::BN * kEdwLDK * sizeof(unsigned short);
  const size_t ms_bytes = (size_t)Tl::CM * g.plane * sizeof(unsigned short);
  const size_t lds = xs_bytes > ms_bytes ? xs_bytes : ms_bytes;
  if (lds > kEdwMaxLds) return MTR_E_SHAPE;
  const long long images = g.xcd_map ? (a.B + 7) / 8 * 8 : a.B;
  const long long gx = images * g.chunks;
  if (gx > 0x7fffffffLL) return MTR_E_SHAPE;
  if (!a.y) return (int)lds;
  auto kern = expand_dw16_kernel<DT, NPT>;
  if (lds > 64 * 1024) {
    const int e = allow_dynamic_lds((const void*)kern, kEdwMaxLds);
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
static int launch_expand_dw16(const EdwArgs& a, const EdwGeo& g) {
  switch (g.HW) {
    case 256: return launch_expand_dw16_cfg<DT, 8>(a, g);
    case 128: return launch_expand_dw16_cfg<DT, 4>(a, g);
    case 64: return launch_expand_dw16_cfg<DT, 2>(a, g);
    default: return launch_expand_dw16_cfg<DT, 1>(a, g);  // 32 and 16 positions: one tile, rows past HW zero
  }
}

}  // namespace mtr

extern "C" size_t mtr_expand_dw16_lds_bytes(long long B, int Cin, int Cmid, int H, int W) {
  mtr::EdwGeo g;
  if (B <= 0 || mtr::expand_dw16_shape(g, B, Cin, Cmid, H, W) != MTR_OK) return 0;
  // (the tile and LDS rules do not depend on the dtype)
  mtr::EdwArgs a = {};
  a.B = B;
  const int n = mtr::launch_expand_dw16<MTR_F16>(a, g);
  return n > 0 ? (size_t)n : 0;
}

extern "C" int mtr_expand_dw16_opts(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                                    const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin,
                                    int Cmid, int H, int W, void* y, float* row_mean, mtr_stream_t stream,
                                    int mapping) {
  if (!x || !w1 || !bias1 || !w_dw || !bias_dw || !y) return MTR_E_NULL;
  if (dtype != MTR_F16 && dtype != MTR_BF16) return MTR_E_DTYPE;
  mtr::EdwGeo g;
  const int e = mtr::expand_dw16_shape(g, B, Cin, Cmid, H, W);
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
  const mtr::EdwArgs a = {x, w1, bias1, w_dw, bias_dw, y, row_mean, act1_code, act2_code, B, (hipStream_t)stream};
  const int rc = dtype == MTR_F16 ? mtr::launch_expand_dw16<MTR_F16>(a, g) : mtr::launch_expand_dw16<MTR_BF16>(a, g);
  return rc;
}

extern "C" int mtr_expand_dw16(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                               const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin, int Cmid,
                               int H, int W, void* y, float* row_mean, mtr_stream_t stream) {
  return mtr_expand_dw16_opts(x, dtype, w1, bias1, act1_code, w_dw, bias_dw, act2_code, B, Cin, Cmid, H, W, y,
                              row_mean, stream, -1);
}
