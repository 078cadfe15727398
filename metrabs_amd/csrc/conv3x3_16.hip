// K14h: a dense 3x3 convolution (stride 1 or 2, padding 1, groups 1) of f16 / bf16 NCHW tensors as one
// implicit 16-bit MFMA GEMM with the K10 epilogue folded in.
//
// Not part of the reference's hot path (like K10 - K13h): the FusedMBConv 3x3 layers of the backbone's 16-bit
// inference copy (backbones.fold_batchnorm(fused_epilogue=True, dtype=f16 / bf16)).  PyTorch-ROCm runs each
// as a MIOpen convolution, then K10.  Here, in one launch:
//
//   y[b, m, oy, ox] = rnd16(act(bias[m] + sum_{ky, kx, ci} W[m, ky, kx, ci] * x[b, ci, s oy + ky - 1, s ox + kx - 1])
//                           (+ residual[b, m, oy, ox]))
//
// accumulated in f32, the epilogue in f32 in K10's order (bias, activation, then the residual), rounded to 16
// bits once.  The reduction index is k = (ky, kx, ci) with ci innermost, 9 Cin long, which is why the weight
// comes repacked as [Cout][3][3][Cin]: eight consecutive k are eight consecutive input channels at one tap.
//
// One workgroup computes BM output channels of a TH x TW tile of output positions of one image (TH TW = BN).
//   * Input: the tile's whole halo, ((TH - 1) s + 3) rows of all Cin channels, is staged ONCE into LDS as an
//     [row][column][ci] image, transposed on the way in: a loader unit reads 4 channel rows x 4 columns (four
//     8-byte loads) and writes 4 positions x 4 ci (four 8-byte LDS writes).  The units are 4-column groups
//     aligned to the input row (W % 4 == 0), so a unit lies wholly inside or wholly outside the image: the
//     padding ring is zero-filled in LDS and the k loop has no bounds tests.  The staged columns start at
//     s ox0 - 4, the aligned group that holds the left halo column.
//     A position's row is Cin (+ 8 when Cin % 16 == 0) elements long: consecutive positions are then an odd
//     number of 16-byte bank groups apart, and the 16-byte fragment reads of 16 consecutive positions hit
//     distinct banks (stride 1; two-way at stride 2).
//   * The k loop walks 16-k MFMA steps (v_mfma_f32_32x32x16_{f16,bf16}, the operand maps of K13h): lane (r, h)
//     = (lane & 31, lane >> 5) holds the 8-k group g = 2 step + h of position r (A) and of weight row r (B).
//     Group g is tap g / (Cin / 8), channels 8 (g % (Cin / 8)) ...: for A one 16-byte LDS read at the tap's
//     offset from the lane's position, for B one 16-byte global load at W[m][8 g] (L2-resident, prefetched two
//     steps ahead).  9 Cin / 8 may be odd (Cin = 24, 40): the last step's upper half is zero on both operands.
//   * Every lane of an accumulator holds four consecutive output columns of one channel.  The epilogue is applied
//     in registers (one 8-byte residual load per group); the rounded tile is then turned through LDS so that
//     each store instruction writes long runs of a few channel rows, not 16-byte pieces of 32 rows.
//
// The k order is the same for every tile shape and configuration -- steps 0, 1, 2, ... of the one (ky, kx, ci)
// sequence -- so the result does not depend on the tile picked.  No atomics, no split-K: the same inputs
// give the same bits.
#include "common.h"

namespace mtr {

typedef float c3_f32x16 __attribute__((ext_vector_type(16)));

template <int DT> struct Conv3Bits;
template <> struct Conv3Bits<MTR_F16> {
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ float f32(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
  static __device__ __forceinline__ c3_f32x16 mfma(uint4 a, uint4 b, c3_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};
template <> struct Conv3Bits<MTR_BF16> {
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ float f32(unsigned short b) { return (float)__builtin_bit_cast(__bf16, b); }
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
  static __device__ __forceinline__ c3_f32x16 mfma(uint4 a, uint4 b, c3_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};

// the geometry of one launch, computed on the host (conv3x3_geometry) and used by both sides
struct Conv3Geo {
  int Cin, M, H, W, Ho, Wo, stride;
  int lw;        // log2 of the tile width TW; TH = BN >> lw
  int tiles_x;   // tiles per output row
  int HH, LW;    // staged halo: rows, columns (a multiple of 4)
  int LDC;       // elements per staged position
};

constexpr int kConv3LoadUnroll = 4;  // loader units in flight per thread
constexpr int kConv3Prefetch = 2;    // k steps of weight fragments in flight per lane (4 measured no faster)

// WM x WN waves, each FM x FN tiles of 32 x 32 (channels x positions)
template <int DT, int WM, int WN, int FM, int FN>
__global__ __launch_bounds__(64 * WM * WN) void conv3x3_16_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w, const float* __restrict__ bias,
    const unsigned short* __restrict__ residual, unsigned short* __restrict__ y, Conv3Geo g, int act) {
  using Hh = Conv3Bits<DT>;
  constexpr int NT = 64 * WM * WN;
  constexpr int BM = 32 * FM * WM, BN = 32 * FN * WN;
  constexpr int U = kConv3LoadUnroll;
  extern __shared__ __attribute__((aligned(16))) unsigned short xs[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int r = lane & 31, h = lane >> 5;
  const int Cin = g.Cin, M = g.M, H = g.H, W = g.W, s = g.stride, LW = g.LW, LDC = g.LDC;
  const int TW = 1 << g.lw;
  const int tile_y = blockIdx.x / g.tiles_x, tile_x = blockIdx.x - tile_y * g.tiles_x;
  const int oy0 = tile_y * (BN >> g.lw), ox0 = tile_x * TW, m0 = blockIdx.y * BM;
  const long long b = blockIdx.z, plane = (long long)H * W;

  // ---- stage the halo: [HH rows][LW columns][Cin], input rows oy0 s - 1 ..., input columns ox0 s - 4 ...
  {
    const unsigned short* xb = x + b * Cin * plane;
    const int iy0 = oy0 * s - 1, ix0 = ox0 * s - 4;
    const int GW = LW >> 2, n_units = 4 * GW * g.HH * ((Cin + 15) >> 4);
    for (int u0 = 0; u0 < n_units; u0 += U * NT) {
      uint2 v[U][4];
      int dst[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        // unit -> (4 channels c4, halo row ly, column group gx): four channel quads, then the column groups
        // of a row, are neighbours in the wave (64-byte runs of a channel row per 32 lanes)
        const int u = u0 + k * NT + tid;
        dst[k] = -1;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[k][i] = make_uint2(0u, 0u);
        if (u < n_units) {
          const int rest = u >> 2, gx = rest % GW, rest2 = rest / GW, ly = rest2 % g.HH;
          const int c4 = (rest2 / g.HH) * 4 + (u & 3);
          if (4 * c4 < Cin) {
            dst[k] = (ly * LW + 4 * gx) * LDC + 4 * c4;
            const int iy = iy0 + ly, ix = ix0 + 4 * gx;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) {  // (W % 4 == 0: the whole group is inside)
              const unsigned short* p = xb + (long long)(4 * c4) * plane + (long long)iy * W + ix;
#pragma unroll
              for (int i = 0; i < 4; ++i) v[k][i] = *reinterpret_cast<const uint2*>(p + i * plane);
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        if (dst[k] < 0) continue;
        unsigned short* d = xs + dst[k];
        uint2 o;  // 4 channel rows x 4 columns -> 4 positions x 4 ci
        o.x = (v[k][0].x & 0xffffu) | (v[k][1].x << 16);
        o.y = (v[k][2].x & 0xffffu) | (v[k][3].x << 16);
        *reinterpret_cast<uint2*>(d) = o;
        o.x = (v[k][0].x >> 16) | (v[k][1].x & 0xffff0000u);
        o.y = (v[k][2].x >> 16) | (v[k][3].x & 0xffff0000u);
        *reinterpret_cast<uint2*>(d + LDC) = o;
        o.x = (v[k][0].y & 0xffffu) | (v[k][1].y << 16);
        o.y = (v[k][2].y & 0xffffu) | (v[k][3].y << 16);
        *reinterpret_cast<uint2*>(d + 2 * LDC) = o;
        o.x = (v[k][0].y >> 16) | (v[k][1].y & 0xffff0000u);
        o.y = (v[k][2].y >> 16) | (v[k][3].y & 0xffff0000u);
        *reinterpret_cast<uint2*>(d + 3 * LDC) = o;
      }
    }
  }

  // ---- the k loop: groups of 8 k, two per MFMA step
  const int G8 = Cin >> 3, NG = 9 * G8, n_steps = (NG + 1) >> 1;
  const long long K9 = 9LL * Cin;
  int abase[FN];  // this lane's position of each tile, at tap (0, 0): element offset into xs
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int p = (wn * FN + j) * 32 + r, oyl = p >> g.lw, oxl = p & (TW - 1);
    abase[j] = ((oyl * s) * LW + oxl * s + 3) * LDC;
  }
  const unsigned short* wrow[FM];  // this lane's weight rows (rows past Cout: row 0, never stored)
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + (wm * FM + i) * 32 + r;
    wrow[i] = w + (m < M ? m : 0) * K9;
  }
  // (no branch around the load: past the last group it re-reads the last one, and the step zeroes what it uses)
  auto load_w = [&](uint4 (&wr)[FM], int grp) {
    const int gq = grp < NG ? grp : NG - 1;
#pragma unroll
    for (int i = 0; i < FM; ++i) wr[i] = *reinterpret_cast<const uint4*>(wrow[i] + 8 * gq);
  };

  c3_f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  int grp = h, tap = h / G8, c8 = h - tap * G8;  // this lane's group of the current step
  // the weight fragments of the next D steps are in flight (a ring of D register sets, the loop unrolled D
  // times so that every index is static): an L2 hit takes several steps' worth of MFMAs
  constexpr int D = kConv3Prefetch;
  uint4 wq[D][FM];
#pragma unroll
  for (int d = 0; d < D; ++d) load_w(wq[d], grp + 2 * d);
  __syncthreads();
  for (int step = 0; step < n_steps; step += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (step + d >= n_steps) break;
      const bool valid = grp < NG;
      const int ky = tap / 3, kx = tap - 3 * ky;
      const int toff = valid ? (ky * LW + kx) * LDC + 8 * c8 : 0;
      uint4 a[FN];
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        a[j] = *reinterpret_cast<const uint4*>(xs + abase[j] + toff);
        if (!valid) a[j] = make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const uint4 wv = valid ? wq[d][i] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = Hh::mfma(a[j], wv, acc[i][j]);
      }
      load_w(wq[d], grp + 2 * D);
      grp += 2;
      c8 += 2;
      if (c8 >= G8) { c8 -= G8; ++tap; }
      if (c8 >= G8) { c8 -= G8; ++tap; }
    }
  }

  // ---- epilogue: lane holds channel m = .. + r, positions 32 j + 8 q + 4 h + 0..3 of the wave's 32 FN.  Bias,
  // activation and the skip are applied in registers; the rounded 32 x 32 FN tile then goes through this wave's
  // own LDS rows ([channel][position], LDP apart: conflict-free 8-byte writes) so that the global stores run
  // along the rows: 8 FN neighbouring lanes write one channel's 64 FN contiguous bytes (with TW = 64 a whole
  // 128-byte line) instead of 32 channels' 16-byte pieces per instruction.
  constexpr int LDP = 32 * FN + 4;
  __syncthreads();  // every wave has read its last halo fragment: the halo's LDS is free
  unsigned short* ys = xs + wave * (32 * LDP);
  auto epilogue = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
    constexpr int PL = 8 * FN, CH = 64 / PL;  // lanes per channel row, channel rows per store instruction
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int mb = m0 + (wm * FM + i) * 32, m = mb + r;
      const float bm = m < M ? bias[m] : 0.0f;
      const long long chan = (b * M + m) * (long long)g.Ho * g.Wo;
#pragma unroll
      for (int j = 0; j < FN; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = activate<ACT>(acc[i][j][4 * q + e] + bm);
          if (residual) {  // the block's skip connection, added after the activation (K10's order)
            const int p = (wn * FN + j) * 32 + 8 * q + 4 * h;
            const int oy = oy0 + (p >> g.lw), ox = ox0 + (p & (TW - 1));
            if (m < M && oy < g.Ho && ox < g.Wo) {  // (Wo % 4 == 0: the whole group is inside)
              const uint2 t = *reinterpret_cast<const uint2*>(residual + chan + (long long)oy * g.Wo + ox);
              v[0] += Hh::f32((unsigned short)(t.x & 0xffffu));
              v[1] += Hh::f32((unsigned short)(t.x >> 16));
              v[2] += Hh::f32((unsigned short)(t.y & 0xffffu));
              v[3] += Hh::f32((unsigned short)(t.y >> 16));
            }
          }
          uint2 o;
          o.x = (unsigned)Hh::rnd(v[0]) | ((unsigned)Hh::rnd(v[1]) << 16);
          o.y = (unsigned)Hh::rnd(v[2]) | ((unsigned)Hh::rnd(v[3]) << 16);
          *reinterpret_cast<uint2*>(ys + r * LDP + 32 * j + 8 * q + 4 * h) = o;
        }
      }
      __syncthreads();
#pragma unroll
      for (int pass = 0; pass < 32 / CH; ++pass) {
        const int c = pass * CH + lane / PL, pp = (lane % PL) * 4;
        const uint2 o = *reinterpret_cast<const uint2*>(ys + c * LDP + pp);
        const int p = wn * FN * 32 + pp;
        const int oy = oy0 + (p >> g.lw), ox = ox0 + (p & (TW - 1));
        if (mb + c < M && oy < g.Ho && ox < g.Wo)
          *reinterpret_cast<uint2*>(y + ((b * M + mb + c) * g.Ho + oy) * (long long)g.Wo + ox) = o;
      }
      if (i + 1 < FM) __syncthreads();  // the rows are rewritten by the next channel tile
    }
  };
  // wave-uniform: one epilogue body per activation, the GEMM shared.  Written out: behind the shared with_act() the
  // compiler lays the epilogue's branches out another way and two instantiations take two SGPRs more (DESIGN.md
  // section 27)
  switch (act) {
    case kActRelu: epilogue(ActTag<kActRelu>()); break;
    case kActSilu: epilogue(ActTag<kActSilu>()); break;
    case kActHardswish: epilogue(ActTag<kActHardswish>()); break;
    default: epilogue(ActTag<kActNone>()); break;
  }
}

constexpr size_t kConv3MaxLds = 160 * 1024;

// The tile width TW in {64, 32, 16, 8} (TH = BN / TW) that pads the output map least; the wider one on a tie.
inline void conv3x3_geometry(Conv3Geo& g, int BN) {
  long long best = -1;
  for (int lw = 6; lw >= 3; --lw) {
    const int TW = 1 << lw, TH = BN >> lw;
    const long long padded = (long long)((g.Wo + TW - 1) / TW) * TW * (((g.Ho + TH - 1) / TH) * TH);
    if (best < 0 || padded < best) {
      best = padded;
      g.lw = lw;
    }
  }
  const int TW = 1 << g.lw, TH = BN >> g.lw;
  g.tiles_x = (g.Wo + TW - 1) / TW;
  g.HH = (TH - 1) * g.stride + 3;
  g.LW = 4 * (((TW - 1) * g.stride + 6 + 3) / 4);
  g.LDC = g.Cin + ((g.Cin & 8) ? 0 : 8);
}

template <int DT, int WM, int WN, int FM, int FN>
static int launch_conv3x3_16_cfg(const void* x, const void* w, const float* bias, const void* residual, void* y,
                                 int act, long long B, Conv3Geo g, hipStream_t stream) {
  constexpr int BM = 32 * FM * WM, BN = 32 * FN * WN;
  conv3x3_geometry(g, BN);
  size_t lds = (size_t)g.HH * g.LW * g.LDC * sizeof(unsigned short);
  if (lds > kConv3MaxLds) return MTR_E_SHAPE;  // the halo of all Cin channels does not fit: the library path
  lds = std::max(lds, (size_t)(WM * WN) * 32 * (32 * FN + 4) * sizeof(unsigned short));  // the epilogue's rows
  const int TH = BN >> g.lw;
  const long long gx = (long long)g.tiles_x * ((g.Ho + TH - 1) / TH), gy = (g.M + BM - 1) / BM;
  if (gx > 0x7fffffffLL || gy > 65535 || B > 65535) return MTR_E_SHAPE;
  if (!y) return (int)lds;  // the shape query (mtr_conv3x3_16_lds_bytes): no launch
  auto kern = conv3x3_16_kernel<DT, WM, WN, FM, FN>;
  if (lds > 64 * 1024) {
    const int e = allow_dynamic_lds((const void*)kern, kConv3MaxLds);
    if (e != MTR_OK) return e;
  }
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)B), block(64 * WM * WN);
  MTR_CLEAR_STALE();
  hipLaunchKernelGGL(kern, grid, block, lds, stream, (const unsigned short*)x, (const unsigned short*)w, bias,
                     (const unsigned short*)residual, (unsigned short*)y, g, act);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

// The configuration table, chosen from Cout only; 4 waves each:
//   Cout <= 32 : 1 x 4 waves of 1 x 2 tiles:  32 channels x 256 positions (stage 1: every x element read once)
//   Cout <= 96 : 1 x 4 waves of 3 x 1 tiles:  96 x 128
//   Cout 129 .. 192 or a multiple of 192: 2 x 2 waves of 3 x 2 tiles: 192 x 128
//   otherwise  : 2 x 2 waves of 2 x 2 tiles: 128 x 128, ceil(Cout / 128) workgroups per position tile
template <int DT>
static int launch_conv3x3_16(const void* x, const void* w, const float* bias, const void* residual, void* y, int act,
                             long long B, const Conv3Geo& g, hipStream_t s) {
  const int M = g.M;
  if (M <= 32) return launch_conv3x3_16_cfg<DT, 1, 4, 1, 2>(x, w, bias, residual, y, act, B, g, s);
  if (M <= 96) return launch_conv3x3_16_cfg<DT, 1, 4, 3, 1>(x, w, bias, residual, y, act, B, g, s);
  if ((M > 128 && M <= 192) || M % 192 == 0)
    return launch_conv3x3_16_cfg<DT, 2, 2, 3, 2>(x, w, bias, residual, y, act, B, g, s);
  return launch_conv3x3_16_cfg<DT, 2, 2, 2, 2>(x, w, bias, residual, y, act, B, g, s);
}

// the shape rules of the entry (MTR_E_SHAPE: the caller takes the library path); fills g
static int conv3x3_16_shape(Conv3Geo& g, long long B, int Cin, int Cout, int H, int W, int stride) {
  if (B < 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (stride != 1 && stride != 2) return MTR_E_SHAPE;
  // 16-byte groups of 8 input channels; 8-byte groups of 4 columns of x, y and the residual
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if (Cin % 8 || W % 4 || Wo % 4) return MTR_E_SHAPE;
  if ((long long)Cin * H * W > 0x7fffffffLL || (long long)Cout * Ho * Wo > 0x7fffffffLL || Cin > 4096)
    return MTR_E_SHAPE;
  g = Conv3Geo{};
  g.Cin = Cin, g.M = Cout, g.H = H, g.W = W, g.Ho = Ho, g.Wo = Wo, g.stride = stride;
  return MTR_OK;
}

}  // namespace mtr

extern "C" size_t mtr_conv3x3_16_lds_bytes(long long B, int Cin, int Cout, int H, int W, int stride) {
  mtr::Conv3Geo g;
  if (mtr::conv3x3_16_shape(g, B, Cin, Cout, H, W, stride) != MTR_OK) return 0;
  // (the tile and LDS rules do not depend on the dtype)
  const int n = mtr::launch_conv3x3_16<MTR_F16>(nullptr, nullptr, nullptr, nullptr, nullptr, 0, B, g, nullptr);
  return n > 0 ? (size_t)n : 0;
}

extern "C" int mtr_conv3x3_bias_act16(const void* x, int dtype, const void* weight, const float* bias,
                                      const void* residual, int act, long long B, int Cin, int Cout, int H, int W,
                                      int stride, void* y, mtr_stream_t stream) {
  if (!x || !weight || !bias || !y) return MTR_E_NULL;
  if (dtype != MTR_F16 && dtype != MTR_BF16) return MTR_E_DTYPE;
  mtr::Conv3Geo g;
  const int e = mtr::conv3x3_16_shape(g, B, Cin, Cout, H, W, stride);
  if (e != MTR_OK) return e;
  if (act < mtr::kActNone || act > mtr::kActHardswish) return MTR_E_PARAM;
  if (((uintptr_t)x % 16) || ((uintptr_t)weight % 16) || ((uintptr_t)y % 16) || ((uintptr_t)residual % 16) ||
      ((uintptr_t)bias % 4))
    return MTR_E_ALIGN;
  if (x == y || residual == y) return MTR_E_PARAM;  // y is written while x and the residual are still read
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return mtr_conv3x3_16_lds_bytes(1, Cin, Cout, H, W, stride) ? MTR_OK : MTR_E_SHAPE;  // nothing to do
  if (dtype == MTR_F16) return mtr::launch_conv3x3_16<MTR_F16>(x, weight, bias, residual, y, act, B, g, s);
  return mtr::launch_conv3x3_16<MTR_BF16>(x, weight, bias, residual, y, act, B, g, s);
}
