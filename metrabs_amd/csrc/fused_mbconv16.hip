// K16h: a whole FusedMBConv block of the 16-bit inference copy -- the dense 3x3 expand (K14h, conv3x3_16.hip) and the
// 1x1 project behind it (K13h, conv1x1_16.hip) -- as ONE launch, the 4x-wide activation between them kept in LDS.
//
//   mid[b, c, p] = rnd16(act(bias3[c] + conv3x3(x, W3, stride, pad 1)[b, c, p]))              c < Cmid
//   y[b, m, p]   = rnd16(bias1[m] + sum_c W1[m, c] * mid[b, c, p] (+ residual[b, m, p]))       m < Cout
//
// Not part of the reference's hot path (like K10 - K15).  The contract is the bits of the two-kernel chain: both
// of its kernels accumulate in a k order that does not depend on the tile -- 16-k MFMA steps of the one
// (ky, kx, ci) sequence, then 16-k steps at c = 0, 16, 32, ..., lane (r, h) holding the 8-k group 2 step + h -- so
// this kernel walks the same steps with the same k slots, rounds `mid` as K14h rounds its output (plain casts),
// and applies the epilogues in the same order (bias, activation; bias, then the skip).
//
// One workgroup of 4 waves computes ALL Cout channels of a TH x TW tile of 128 output positions of one image.
//   * The input halo of the tile is staged once, exactly as in K14h: [row][column][ci], transposed on the way
//     in, the padding ring zero-filled in LDS, no bounds test in the k loop.
//   * Cmid is walked in chunks of 64 FM channels (FM = 2 or 3: 128 or 192), ascending.  Per chunk:
//       1. the expand's full 9 Cin k loop, 2 x 2 waves of FM x 2 tiles of 32 x 32 (K14h's loop: weight
//          fragments 16-byte loads of W3[c][8 g] from L2, two steps ahead).  The MFMA operands are SWAPPED
//          against K14h -- weights as A, positions as B: the same products in the same k slots, but a lane
//          then holds four consecutive CHANNELS of one position instead of four positions of one channel;
//       2. bias, activation, rounding, in registers;
//       3. the chunk goes to LDS as a [position][c] image with 8-byte writes (rows CHUNK + 8 elements long:
//          K13h's X^T image, conflict-free 16-byte fragment reads);
//       4. the chunk's part of the project: each wave owns 32 positions and all Cout channels (FMO tiles of
//          32), CHUNK / 16 MFMA steps in K13h's operand order, W1 fragments 16-byte loads of W1[m][8 g] from
//          L2, two steps ahead.  Channels past Cmid are zero in the image and in the fragment.
//   * The project's epilogue is applied in registers (bias, the skip by one 8-byte load per group); the rounded
//     Cout x 128 tile is then turned through LDS so that 16 neighbouring lanes write one channel row's run.
// No atomics, no split-K, no workspace: the same inputs give the same bits, whichever FM / FMO the shape picks.
#include "common.h"

namespace mtr {

typedef float fmb_f32x16 __attribute__((ext_vector_type(16)));

template <int DT> struct FmbBits;
template <> struct FmbBits<MTR_F16> {
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ float f32(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
  static __device__ __forceinline__ fmb_f32x16 mfma(uint4 a, uint4 b, fmb_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};
template <> struct FmbBits<MTR_BF16> {
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ float f32(unsigned short b) { return (float)__builtin_bit_cast(__bf16, b); }
  static __device__ __forceinline__ unsigned short rnd(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }
  static __device__ __forceinline__ fmb_f32x16 mfma(uint4 a, uint4 b, fmb_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8, a), __builtin_bit_cast(v8, b), c, 0, 0, 0);
  }
};

// the geometry of one launch, computed on the host (fmb_geometry) and used by both sides
struct FmbGeo {
  int Cin, Cmid, Cout, H, W, Ho, Wo, stride;
  int lw;        // log2 of the tile width TW; TH = 128 >> lw
  int tiles_x;   // tiles per output row
  int HH, LW;    // staged halo: rows, columns (a multiple of 4)
  int LDC;       // elements per staged position
  int halo;      // elements of the staged halo: the chunk image starts behind it
};

constexpr int kFmbBN = 128;        // output positions per workgroup
constexpr int kFmbLoadUnroll = 4;  // loader units in flight per thread
constexpr int kFmbPrefetch = 2;    // k steps of weight fragments in flight per lane
constexpr int kFmbLDP = kFmbBN + 4;  // elements per channel row of the output tile in LDS

// FM: 32-channel tiles of the expand per wave (chunk = 64 FM channels); FMO: 32-channel tiles of the project
template <int DT, int FM, int FMO>
__global__ __launch_bounds__(256) void fused_mbconv16_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w3, const float* __restrict__ bias3,
    const unsigned short* __restrict__ w1, const float* __restrict__ bias1,
    const unsigned short* __restrict__ residual, unsigned short* __restrict__ y, FmbGeo g, int act) {
  using Hh = FmbBits<DT>;
  constexpr int NT = 256, WM = 2, FN = 2;
  constexpr int CHUNK = 64 * FM, LDM = CHUNK + 8, KS = CHUNK / 16;
  constexpr int U = kFmbLoadUnroll, D = kFmbPrefetch, LDP = kFmbLDP;
  extern __shared__ __attribute__((aligned(16))) unsigned short xs[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int r = lane & 31, h = lane >> 5;
  const int Cin = g.Cin, Cmid = g.Cmid, Cout = g.Cout, H = g.H, W = g.W, s = g.stride, LW = g.LW, LDC = g.LDC;
  const int TW = 1 << g.lw;
  const int tile_y = blockIdx.x / g.tiles_x, tile_x = blockIdx.x - tile_y * g.tiles_x;
  const int oy0 = tile_y * (kFmbBN >> g.lw), ox0 = tile_x * TW;
  const long long b = blockIdx.z, plane = (long long)H * W;
  unsigned short* ms = xs + g.halo;  // the chunk image [128 positions][LDM]; at the end the output tile

  // ---- stage the halo: [HH rows][LW columns][Cin], input rows oy0 s - 1 ..., input columns ox0 s - 4 ... (K14h's)
  {
    const unsigned short* xb = x + b * Cin * plane;
    const int iy0 = oy0 * s - 1, ix0 = ox0 * s - 4;
    const int GW = LW >> 2, n_units = 4 * GW * g.HH * ((Cin + 15) >> 4);
    for (int u0 = 0; u0 < n_units; u0 += U * NT) {
      uint2 v[U][4];
      int dst[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
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

  const int G8 = Cin >> 3, NG = 9 * G8, n_steps = (NG + 1) >> 1;
  const long long K9 = 9LL * Cin;
  int abase[FN];  // this lane's position of each expand tile, at tap (0, 0): element offset into xs
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int p = (wn * FN + j) * 32 + r, oyl = p >> g.lw, oxl = p & (TW - 1);
    abase[j] = ((oyl * s) * LW + oxl * s + 3) * LDC;
  }
  // the project: this wave's 32 positions, this lane's W1 rows (rows past Cout: row 0, never stored)
  const unsigned short* w1row[FMO];
#pragma unroll
  for (int io = 0; io < FMO; ++io) {
    const int m = 32 * io + r;
    w1row[io] = w1 + (long long)(m < Cout ? m : 0) * Cmid;
  }
  // (no branch around the load: past Cmid it re-reads the row's last group and zeroes the fragment)
  auto load_w1 = [&](uint4 (&wr)[FMO], int k) {
    const bool valid = k < Cmid;
    const int kq = valid ? k : Cmid - 8;
#pragma unroll
    for (int io = 0; io < FMO; ++io) {
      const uint4 t = *reinterpret_cast<const uint4*>(w1row[io] + kq);
      wr[io] = valid ? t : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  fmb_f32x16 pacc[FMO];
#pragma unroll
  for (int io = 0; io < FMO; ++io)
#pragma unroll
    for (int e = 0; e < 16; ++e) pacc[io][e] = 0.0f;

  __syncthreads();  // the halo is staged

  for (int c0 = 0; c0 < Cmid; c0 += CHUNK) {
    // ---- 1. the expand of channels c0 .. c0 + CHUNK - 1: K14h's k loop, operands swapped
    const unsigned short* wrow[FM];  // this lane's weight rows (rows past Cmid: row 0, zeroed in the image)
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int m = c0 + (wm * FM + i) * 32 + r;
      wrow[i] = w3 + (m < Cmid ? m : 0) * K9;
    }
    // (no branch around the load: past the last group it re-reads the last one, and the step zeroes what it uses)
    auto load_w = [&](uint4 (&wr)[FM], int grp) {
      const int gq = grp < NG ? grp : NG - 1;
#pragma unroll
      for (int i = 0; i < FM; ++i) wr[i] = *reinterpret_cast<const uint4*>(wrow[i] + 8 * gq);
    };
    fmb_f32x16 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

    int grp = h, tap = h / G8, c8 = h - tap * G8;  // this lane's group of the current step
    uint4 wq[D][FM];
#pragma unroll
    for (int d = 0; d < D; ++d) load_w(wq[d], grp + 2 * d);
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
          for (int j = 0; j < FN; ++j) acc[i][j] = Hh::mfma(wv, a[j], acc[i][j]);
        }
        load_w(wq[d], grp + 2 * D);
        grp += 2;
        c8 += 2;
        if (c8 >= G8) { c8 -= G8; ++tap; }
        if (c8 >= G8) { c8 -= G8; ++tap; }
      }
    }

    // the first W1 fragments of this chunk: in flight behind the expand's epilogue
    uint4 wq1[2][FMO];
    load_w1(wq1[0], c0 + 8 * h);
    load_w1(wq1[1], c0 + 16 + 8 * h);

    // ---- 2. + 3. lane holds position .. + r, channels 32 i + 8 q + 4 h + 0..3 of the wave's 32 FM: bias,
    // activation, rounding (what K14h stores), then one 8-byte write into the [position][c] image
    __syncthreads();  // every wave has read the previous chunk's image
    auto to_image = [&](auto tag) {
      constexpr int ACT = decltype(tag)::value;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int cl = (wm * FM + i) * 32 + 8 * q + 4 * h, c = c0 + cl;
          const bool in = c < Cmid;  // (Cmid % 8 == 0: the whole group is inside or outside)
          const float* bp = bias3 + (in ? c : 0);
          const float bq[4] = {bp[0], bp[1], bp[2], bp[3]};
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            float v[4];
            // (settled: the activation's last product is rounded to f32 before it is rounded to 16 bits, as the
            // stored output of K14h is -- not contracted into the conversion)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = settled(activate<ACT>(acc[i][j][4 * q + e] + bq[e]));
            uint2 o;
            o.x = (unsigned)Hh::rnd(v[0]) | ((unsigned)Hh::rnd(v[1]) << 16);
            o.y = (unsigned)Hh::rnd(v[2]) | ((unsigned)Hh::rnd(v[3]) << 16);
            if (!in) o = make_uint2(0u, 0u);
            *reinterpret_cast<uint2*>(ms + ((wn * FN + j) * 32 + r) * LDM + cl) = o;
          }
        }
      }
    };
    // wave-uniform: one body per activation, the GEMMs shared.  Written out: behind the shared with_act() a few
    // instructions trade places inside the chunk loop
    switch (act) {
      case kActRelu: to_image(ActTag<kActRelu>()); break;
      case kActSilu: to_image(ActTag<kActSilu>()); break;
      case kActHardswish: to_image(ActTag<kActHardswish>()); break;
      default: to_image(ActTag<kActNone>()); break;
    }
    __syncthreads();

    // ---- 4. the chunk's part of the project: K13h's steps at c0, c0 + 16, ...
    const unsigned short* xa = ms + (wave * 32 + r) * LDM + 8 * h;
#pragma unroll
    for (int st = 0; st < KS; ++st) {
      const uint4 a = *reinterpret_cast<const uint4*>(xa + 16 * st);
#pragma unroll
      for (int io = 0; io < FMO; ++io) pacc[io] = Hh::mfma(a, wq1[st & 1][io], pacc[io]);
      if (st + 2 < KS) load_w1(wq1[st & 1], c0 + 16 * (st + 2) + 8 * h);
    }
  }

  // ---- the project's epilogue: lane holds channel 32 io + r, positions 8 q + 4 h + 0..3 of the wave's 32.  Bias and
  // the skip in registers (K13h's order); the rounded tile goes through LDS as [channel][position] rows
  __syncthreads();  // every wave has read the last chunk's image
  const long long oplane = (long long)g.Ho * g.Wo;
#pragma unroll
  for (int io = 0; io < FMO; ++io) {
    const int m = 32 * io + r;
    const float bm = m < Cout ? bias1[m] : 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = wave * 32 + 8 * q + 4 * h;
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = activate<kActNone>(pacc[io][4 * q + e] + bm);
      if (residual) {
        const int oy = oy0 + (p >> g.lw), ox = ox0 + (p & (TW - 1));
        if (m < Cout && oy < g.Ho && ox < g.Wo) {  // (Wo % 4 == 0: the whole group is inside)
          const uint2 t = *reinterpret_cast<const uint2*>(residual + (b * Cout + m) * oplane + (long long)oy * g.Wo + ox);
          v[0] += Hh::f32((unsigned short)(t.x & 0xffffu));
          v[1] += Hh::f32((unsigned short)(t.x >> 16));
          v[2] += Hh::f32((unsigned short)(t.y & 0xffffu));
          v[3] += Hh::f32((unsigned short)(t.y >> 16));
        }
      }
      uint2 o;
      o.x = (unsigned)Hh::rnd(v[0]) | ((unsigned)Hh::rnd(v[1]) << 16);
      o.y = (unsigned)Hh::rnd(v[2]) | ((unsigned)Hh::rnd(v[3]) << 16);
      *reinterpret_cast<uint2*>(ms + m * LDP + p) = o;
    }
  }
  __syncthreads();
  // 32 lanes write one channel row's 128 positions (TW = 64: two 128-byte runs), 8 rows per instruction
#pragma unroll
  for (int pass = 0; pass < 4 * FMO; ++pass) {
    const int c = pass * 8 + (tid >> 5), pp = (tid & 31) * 4;
    const uint2 o = *reinterpret_cast<const uint2*>(ms + c * LDP + pp);
    const int oy = oy0 + (pp >> g.lw), ox = ox0 + (pp & (TW - 1));
    if (c < Cout && oy < g.Ho && ox < g.Wo)
      *reinterpret_cast<uint2*>(y + ((b * Cout + c) * g.Ho + oy) * (long long)g.Wo + ox) = o;
  }
}

constexpr size_t kFmbMaxLds = 160 * 1024;

// The tile width TW in {64, 32, 16, 8} (TH = 128 / TW) that pads the output map least; the wider one on a tie
// (K14h's rule at 128 positions), and the staged halo of that tile.
inline void fmb_geometry(FmbGeo& g) {
  long long best = -1;
  for (int lw = 6; lw >= 3; --lw) {
    const int TW = 1 << lw, TH = kFmbBN >> lw;
    const long long padded = (long long)((g.Wo + TW - 1) / TW) * TW * (((g.Ho + TH - 1) / TH) * TH);
    if (best < 0 || padded < best) {
      best = padded;
      g.lw = lw;
    }
  }
  const int TW = 1 << g.lw, TH = kFmbBN >> g.lw;
  g.tiles_x = (g.Wo + TW - 1) / TW;
  g.HH = (TH - 1) * g.stride + 3;
  g.LW = 4 * (((TW - 1) * g.stride + 6 + 3) / 4);
  g.LDC = g.Cin + ((g.Cin & 8) ? 0 : 8);
  g.halo = g.HH * g.LW * g.LDC;
}

template <int DT, int FM, int FMO>
static int launch_fused_mbconv16_cfg(const void* x, const void* w3, const float* bias3, const void* w1,
                                     const float* bias1, const void* residual, void* y, int act, long long B,
                                     const FmbGeo& g, hipStream_t stream) {
  constexpr int CHUNK = 64 * FM;
  static_assert(32 * FMO * kFmbLDP <= kFmbBN * (CHUNK + 8), "the output tile fits the chunk image");
  const size_t lds = ((size_t)g.halo + (size_t)kFmbBN * (CHUNK + 8)) * sizeof(unsigned short);
  if (lds > kFmbMaxLds) return MTR_E_SHAPE;  // halo + chunk image do not fit: the caller keeps the chain
  const int TH = kFmbBN >> g.lw;
  const long long gx = (long long)g.tiles_x * ((g.Ho + TH - 1) / TH);
  if (gx > 0x7fffffffLL || B > 65535) return MTR_E_SHAPE;
  if (!y) return (int)lds;  // the shape query (mtr_fused_mbconv16_lds_bytes): no launch
  auto kern = fused_mbconv16_kernel<DT, FM, FMO>;
  if (lds > 64 * 1024) {
    const int e = allow_dynamic_lds((const void*)kern, kFmbMaxLds);
    if (e != MTR_OK) return e;
  }
  const dim3 grid((unsigned)gx, 1, (unsigned)B), block(256);
  MTR_CLEAR_STALE();
  hipLaunchKernelGGL(kern, grid, block, lds, stream, (const unsigned short*)x, (const unsigned short*)w3, bias3,
                     (const unsigned short*)w1, bias1, (const unsigned short*)residual, (unsigned short*)y, g, act);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

// The configuration, from Cmid and Cout only:
//   FM : chunks of 192 channels where that pads Cmid no more than chunks of 128 do (192, 384, 160), else 128
//   FMO: ceil(Cout / 32) tiles of project accumulators per wave, 2 at least, 4 at most (Cout <= 128)
template <int DT, int FM>
static int launch_fused_mbconv16_fm(const void* x, const void* w3, const float* bias3, const void* w1,
                                    const float* bias1, const void* residual, void* y, int act, long long B,
                                    const FmbGeo& g, hipStream_t s) {
  if (g.Cout <= 64) return launch_fused_mbconv16_cfg<DT, FM, 2>(x, w3, bias3, w1, bias1, residual, y, act, B, g, s);
  if (g.Cout <= 96) return launch_fused_mbconv16_cfg<DT, FM, 3>(x, w3, bias3, w1, bias1, residual, y, act, B, g, s);
  return launch_fused_mbconv16_cfg<DT, FM, 4>(x, w3, bias3, w1, bias1, residual, y, act, B, g, s);
}

template <int DT>
static int launch_fused_mbconv16(const void* x, const void* w3, const float* bias3, const void* w1,
                                 const float* bias1, const void* residual, void* y, int act, long long B,
                                 const FmbGeo& g, hipStream_t s) {
  const int pad2 = (g.Cmid + 127) / 128 * 128, pad3 = (g.Cmid + 191) / 192 * 192;
  if (pad3 <= pad2) return launch_fused_mbconv16_fm<DT, 3>(x, w3, bias3, w1, bias1, residual, y, act, B, g, s);
  return launch_fused_mbconv16_fm<DT, 2>(x, w3, bias3, w1, bias1, residual, y, act, B, g, s);
}

// the shape rules of the entry (MTR_E_SHAPE: the caller keeps the two-kernel chain); fills g
static int fused_mbconv16_shape(FmbGeo& g, long long B, int Cin, int Cmid, int Cout, int H, int W, int stride) {
  if (B < 0 || Cin <= 0 || Cmid <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (stride != 1 && stride != 2) return MTR_E_SHAPE;
  // 16-byte groups of 8 channels of x, W3 and W1; 8-byte groups of 4 columns of x, y and the residual
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  if (Cin % 8 || Cmid % 8 || W % 4 || Wo % 4) return MTR_E_SHAPE;
  if (Cout > 128 || Cin > 4096 || Cmid > 65536) return MTR_E_SHAPE;  // the project's accumulators: 4 tiles per wave
  if ((long long)Cin * H * W > 0x7fffffffLL || (long long)Cout * Ho * Wo > 0x7fffffffLL) return MTR_E_SHAPE;
  g = FmbGeo{};
  g.Cin = Cin, g.Cmid = Cmid, g.Cout = Cout, g.H = H, g.W = W, g.Ho = Ho, g.Wo = Wo, g.stride = stride;
  fmb_geometry(g);
  return MTR_OK;
}

}  // namespace mtr

extern "C" size_t mtr_fused_mbconv16_lds_bytes(long long B, int Cin, int Cmid, int Cout, int H, int W, int stride) {
  mtr::FmbGeo g;
  if (mtr::fused_mbconv16_shape(g, B, Cin, Cmid, Cout, H, W, stride) != MTR_OK) return 0;
  // (the tile and LDS rules do not depend on the dtype)
  const int n = mtr::launch_fused_mbconv16<MTR_F16>(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                                    B, g, nullptr);
  return n > 0 ? (size_t)n : 0;
}

extern "C" int mtr_fused_mbconv16(const void* x, int dtype, const void* w3_packed, const float* bias3, int act,
                                  const void* w1, const float* bias1, const void* residual, long long B, int Cin,
                                  int Cmid, int Cout, int H, int W, int stride, void* y, mtr_stream_t stream) {
  if (!x || !w3_packed || !bias3 || !w1 || !bias1 || !y) return MTR_E_NULL;
  if (dtype != MTR_F16 && dtype != MTR_BF16) return MTR_E_DTYPE;
  mtr::FmbGeo g;
  const int e = mtr::fused_mbconv16_shape(g, B, Cin, Cmid, Cout, H, W, stride);
  if (e != MTR_OK) return e;
  if (residual && (stride != 1 || Cout != Cin)) return MTR_E_SHAPE;  // a skip has the input's shape
  if (act < mtr::kActNone || act > mtr::kActHardswish) return MTR_E_PARAM;
  if (((uintptr_t)x % 16) || ((uintptr_t)w3_packed % 16) || ((uintptr_t)w1 % 16) || ((uintptr_t)y % 16) ||
      ((uintptr_t)residual % 16) || ((uintptr_t)bias3 % 4) || ((uintptr_t)bias1 % 4))
    return MTR_E_ALIGN;
  if (x == y || residual == y) return MTR_E_PARAM;  // y is written while x and the residual are still read
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return mtr_fused_mbconv16_lds_bytes(1, Cin, Cmid, Cout, H, W, stride) ? MTR_OK : MTR_E_SHAPE;
  if (dtype == MTR_F16)
    return mtr::launch_fused_mbconv16<MTR_F16>(x, w3_packed, bias3, w1, bias1, residual, y, act, B, g, s);
  return mtr::launch_fused_mbconv16<MTR_BF16>(x, w3_packed, bias3, w1, bias1, residual, y, act, B, g, s);
}
