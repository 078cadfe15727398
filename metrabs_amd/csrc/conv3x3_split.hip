// K21: a dense 3x3 convolution (stride 1, padding 1, groups 1) of f32 NCHW tensors on the bf16 matrix cores, by
// operand split, with the K10 epilogue folded in.
//
// Not part of the reference's hot path (like K10 - K22): the dense stride-1 3x3 layers of the f32 inference copy
// (backbones.fold_batchnorm(fused_epilogue=True, split3x3=True)).  In one launch:
//
//   y[b, m, oy, ox] = act(bias[m] + sum_{ci, ky, kx} w[m, ci, ky, kx] * x[b, ci, oy + ky - 1, ox + kx - 1])
//                     (+ residual[b, m, oy, ox])
//
// THE ARITHMETIC is K20's (conv1x1_split.hip).  An f32 value is exactly the sum of three bf16 values,
//   a0 = bf16_rn(a), a1 = bf16_rn(a - a0), a2 = bf16_rn(a - a0 - a1)      (the subtractions are exact in f32)
// The weight arrives split (kernels.pack_conv3x3_split_weight): [3][Cout][3][3][Cp] bf16, ci innermost, Cp = Cin
// rounded up to kC3sCK = 16, the tail zero.  x is split on the VALU on its way from global memory into LDS.  Of the
// nine cross products of w = w0 + w1 + w2 and v = v0 + v1 + v2 the six with piece indices summing to at most 2 are
// evaluated, the other three (below 2^-23 |w v|) are dropped.
//
// THE ORDER OF THE SUM.  Every output element has ONE f32 accumulator that starts from 0 and takes the k steps
//
//   for c = 0, 16, 32, ... < Cp:                  (the chunks: kC3sCK = 16 input channels, one constant for all shapes)
//     for ky = 0, 1, 2:  for kx = 0, 1, 2:        (the taps, rows first)
//       for (pw, pv) in (2,0), (0,2), (1,1), (1,0), (0,1), (0,0):       (smallest first, K20's order)
//         acc = v_mfma_f32_32x32x16_bf16(v_pv[b, c .. c + 15, oy + ky - 1, ox + kx - 1], w_pw[m, c .. c + 15, ky, kx], acc)
//
// (x = 0 outside the image and for ci >= Cin).  Then "+ bias", the activation, "+ residual": K10's order (common.h:
// epilogue_store4).  No split-K, no atomics, no workspace.  The sequence does not depend on the tile, the tile's
// position, the configuration, the batch index or whether a residual is given: the same inputs give the same bits
// on every call, every graph replay and every slice of a batch.
//
// Non-finite inputs (K20's caveat): a - bf16(a) of an infinity is NaN, so a window that holds an infinity (or a
// value that rounds to one in bf16, |x| >= 2^127 * (2 - 2^-8)) gives NaN where the library gives an infinity.
//
// Geometry (K14h's, conv3x3_16.hip).  Computed transposed: positions on the MFMA's A rows, output channels on its
// B columns, so a lane ends with four consecutive ox of one channel per register quad: one 16-byte store.  A
// workgroup of four waves owns 256 output positions of one image -- TH x TW, TW = 32 (W > 16) or 16, TH = 256 / TW;
// a position fragment is 32 consecutive positions of the tile, rows first -- and a block of 32 WM FM output
// channels: 32 (Cout <= 32, 1 x 4 waves of 1 x 2 tiles), 64 (Cout <= 64, 2 x 2 waves of 1 x 4), and above that 128
// (2 x 2 waves of 2 x 4) or 96 (1 x 4 waves of 3 x 2), whichever pads Cout less (192 = 2 x 96, 256 = 2 x 128).  The
// sum of an output element is the same in all four.  256 positions, not 128: the weight fragments come from L2 in
// 32-byte pieces of 128-byte lines, and their traffic per MFMA falls with the positions a workgroup covers.
//   * x: Cin is walked in chunks of 16 through LDS, two buffers.  Every thread owns two units of the chunk's halo --
//     4 channels x 4 columns of one of the TH + 2 rows, columns ox0 - 4 .. ox0 + TW + 3 in aligned groups (W % 4 == 0:
//     a group is inside or outside the image as a whole) -- and loads the NEXT chunk's units into registers before
//     this chunk's MFMAs.  Every load is unconditional, from a clamped valid address, and selected against zero on
//     the way into LDS: the padding ring and the channel tail are zeros in LDS and the k loop has no bounds tests.
//   * the LDS image per piece is [halo position p = row * LW + column][16 ci] bf16, 32 bytes per position; the two
//     16-byte halves of a position are swapped where (p >> 3) & 1: the 16 lanes that ds_read_b128 serves in one
//     cycle read 16 positions that differ mod 16 (LW = 40 for TW = 32, LW = 32 for TW = 16), i.e. 16 distinct
//     16-byte slots of the 256-byte bank row.  The A fragment of lane (r, h) = (lane & 31, lane >> 5) is the half h
//     of position r's row at the tap's offset: one ds_read_b128 per piece.
//   * w: the B fragment of lane (r, h) is 16 contiguous bytes of the packed weight, [m][ky][kx][c + 8 h ..], read
//     straight from L2 one tap ahead (two taps ahead in the two configurations with short taps).
//   * one barrier per chunk: the next chunk is written to the other buffer.  Two buffers of three pieces of the halo
//     (400 positions for TW = 32, 576 for TW = 16, 32 bytes each) are 75 / 108 KiB of dynamic LDS.
#include "common.h"

namespace mtr {

typedef float c3s_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 c3s_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kC3sCK = 16;          // input channels per chunk: the 16 k of one v_mfma_f32_32x32x16_bf16
constexpr int kC3sBN = 256;         // output positions per workgroup
constexpr int kC3sXV = 2;           // loader units per thread
constexpr int kC3sMaxPos = 576;     // halo positions of the larger image (TW = 16: 18 rows x 32; TW = 32: 10 x 40)
constexpr size_t kC3sMaxLds = 2 * 3 * (size_t)kC3sMaxPos * kC3sCK * 2;   // 108 KiB

// the geometry of one launch, computed on the host (conv3x3_split_shape)
struct C3sGeo {
  int Cin, Cp, M, H, W;
  int lw;                        // log2 TW
  int LW, HH, GW;                // halo: positions per row of the image, rows, staged 4-column groups per row
  int piece;                     // bytes of one piece of one buffer: HH LW positions of 32 bytes; a buffer is three
  int cfg;                       // 0: 32 channels per workgroup, 1: 64, 2: 128, 3: 96
  unsigned m_blocks, xt, yt;     // channel blocks, tiles per row, tiles per column
  unsigned blocks;               // B yt xt m_blocks
  FastDiv div_mb, div_xt, div_yt, div_gw;
};

// byte offset of (halo position p, 16-byte half q) inside one piece
__device__ __forceinline__ int c3s_slot(int p, int q) { return p * 32 + ((q ^ (p >> 3)) & 1) * 16; }

// WM x WN waves (WM WN = 4), each FM x FN tiles of 32 x 32 (channels x positions); WN FN = 4
template <int WM, int WN, int FM, int FN>
__global__ __launch_bounds__(256, (FM * FN > 2 ? 1 : 2)) void conv3x3_split_kernel(
    const float* __restrict__ x, const uint4* __restrict__ ws, const float* __restrict__ bias,
    const float* __restrict__ residual, float* __restrict__ y, C3sGeo g, int act) {
  static_assert(WM * WN == 4 && WN * FN * 32 == kC3sBN, "four waves, 256 positions");
  extern __shared__ __attribute__((aligned(16))) unsigned char xs[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int r = lane & 31, h = lane >> 5;
  const int Cin = g.Cin, M = g.M, H = g.H, W = g.W, LW = g.LW;
  const int TW = 1 << g.lw;
  const int plane = H * W;

  // ---- the workgroup's tile: channel block fastest (the blocks of one tile read the same x), then the tile of the
  // row, the row of tiles, the image
  unsigned id = blockIdx.x;
  unsigned qd = fastdiv(id, g.div_mb);
  const int m0 = (int)(id - qd * g.m_blocks) * (32 * WM * FM);
  id = qd, qd = fastdiv(id, g.div_xt);
  const int ox0 = (int)(id - qd * g.xt) << g.lw;
  id = qd, qd = fastdiv(id, g.div_yt);
  const int oy0 = (int)(id - qd * g.yt) * (kC3sBN >> g.lw);
  const long long b = qd;

  // ---- the loader's units (the same for every chunk): channel quad cq, halo row ly, column group gx
  const int kPiece = g.piece, kStage = 3 * g.piece;
  const int cq = tid & 3;
  const float* xb = x + b * Cin * plane;
  int xoff[kC3sXV], xdst[kC3sXV];
  bool mine[kC3sXV], inimg[kC3sXV];
#pragma unroll
  for (int j = 0; j < kC3sXV; ++j) {
    const unsigned urest = (unsigned)(tid + 256 * j) >> 2;
    const int ly = (int)fastdiv(urest, g.div_gw), gx = (int)urest - ly * g.GW;
    const int iy = oy0 - 1 + ly, ix = ox0 - 4 + 4 * gx;
    mine[j] = ly < g.HH;
    inimg[j] = mine[j] && iy >= 0 && iy < H && ix >= 0 && ix < W;  // (W % 4 == 0: the whole group)
    xoff[j] = inimg[j] ? iy * W + ix : 0;
    const int p0 = ly * LW + 4 * gx;  // the unit's first halo position; p0 % 4 == 0: its four share (p >> 3) & 1
    xdst[j] = c3s_slot(p0, cq >> 1) + (cq & 1) * 8;
  }

  float4 xv[kC3sXV][4];
  bool xch;
  auto load_chunk = [&](int c0) {
    const int ch = c0 + 4 * cq;
    xch = ch < Cin;                          // (Cin % 8 == 0: a quad never straddles Cin)
    const float* p = xb + (long long)min(ch, Cin - 4) * plane;
#pragma unroll
    for (int j = 0; j < kC3sXV; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[j][i] = *reinterpret_cast<const float4*>(p + (long long)i * plane + xoff[j]);
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int j = 0; j < kC3sXV; ++j) {
      if (!mine[j]) continue;
      const bool xok = inimg[j] && xch;
      unsigned char* d = xs + buf * kStage + xdst[j];
      float v[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        v[i][0] = xok ? xv[j][i].x : 0.0f;
        v[i][1] = xok ? xv[j][i].y : 0.0f;
        v[i][2] = xok ? xv[j][i].z : 0.0f;
        v[i][3] = xok ? xv[j][i].w : 0.0f;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {  // column c of the group: channels 4 cq .. 4 cq + 3 of position p0 + c
        unsigned lo[3], hi[3];
        split_bf16x3_pairs(v[0][c], v[1][c], lo);
        split_bf16x3_pairs(v[2][c], v[3][c], hi);
#pragma unroll
        for (int p = 0; p < 3; ++p) *reinterpret_cast<uint2*>(d + p * kPiece + c * 32) = make_uint2(lo[p], hi[p]);
      }
    }
  };

  // ---- fragment addresses
  int apos[FN];  // this lane's halo position of each fragment at tap (0, 0)
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int q = (wn * FN + j) * 32 + r, oyl = q >> g.lw, oxl = q & (TW - 1);
    apos[j] = oyl * LW + oxl + 3;
  }
  // weight rows: row min(m, M - 1) (a row past Cout feeds only channels that are never stored)
  const int cp8 = g.Cp >> 3;                         // uint4 per (m, tap)
  const long long wpiece = (long long)M * 9 * cp8;   // uint4 per piece
  const uint4* wrow[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = min(m0 + (wm * FM + i) * 32 + r, M - 1);
    wrow[i] = ws + (long long)m * 9 * cp8 + h;
  }
  // the fragments of the next D taps are in flight: one tap where a tap is 36 or 48 MFMAs long, two where it is 12 or
  // 24 (an L2 hit takes longer than 12 MFMAs)
  constexpr int D = FM * FN <= 4 ? 2 : 1;
  uint4 wq[D][FM][3];
  auto load_w = [&](uint4 (&dst)[FM][3], int c0, int t) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) dst[i][p] = wrow[i][p * wpiece + t * cp8 + (c0 >> 3)];
  };

  c3s_f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  const int Cp = g.Cp;
  load_chunk(0);
#pragma unroll
  for (int d = 0; d < D; ++d) load_w(wq[d], 0, d);
  int buf = 0;
  for (int c0 = 0; c0 < Cp; c0 += kC3sCK, buf ^= 1) {
    store_chunk(buf);
    __syncthreads();  // this chunk is in LDS; every wave has left the chunk before, whose buffer is written next
    const int cn = min(c0 + kC3sCK, Cp - kC3sCK);
    load_chunk(cn);   // in flight under this chunk's MFMAs (behind the last chunk: the last one again, dropped)
    const unsigned char* xsb = xs + buf * kStage;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      uint4 wc[FM][3];
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          wc[i][p] = wq[0][i][p];
#pragma unroll
          for (int d = 0; d + 1 < D; ++d) wq[d][i][p] = wq[d + 1][i][p];
        }
      // tap t + D of the one sequence (chunk, tap); behind the last chunk: the last chunk again, dropped
      if (t + D < 9) load_w(wq[D - 1], c0, t + D); else load_w(wq[D - 1], cn, t + D - 9);
      c3s_bf16x8 xa[FN][3];
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int off = c3s_slot(apos[j] + (t / 3) * LW + (t % 3), h);
#pragma unroll
        for (int p = 0; p < 3; ++p) xa[j][p] = *reinterpret_cast<const c3s_bf16x8*>(xsb + p * kPiece + off);
      }
      // the six products, smallest first; (w piece, x piece)
      constexpr int kWp[6] = {2, 0, 1, 1, 0, 0}, kXp[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
      for (int s = 0; s < 6; ++s)
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          const c3s_bf16x8 wb = __builtin_bit_cast(c3s_bf16x8, wc[i][kWp[s]]);
#pragma unroll
          for (int j = 0; j < FN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xa[j][kXp[s]], wb, acc[i][j], 0, 0, 0);
        }
    }
  }

  // ---- epilogue: registers 4 q + e of acc[i][j] are channel m0 + 32 (wm FM + i) + r at the tile's positions
  // 32 (wn FN + j) + 8 q + 4 h + e: four consecutive ox of one output row
  auto epilogue = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int m = m0 + (wm * FM + i) * 32 + r;
      if (m >= M) continue;
      const float bm = bias[m];
      const long long chan = (b * M + m) * (long long)plane;
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int pp = (wn * FN + j) * 32 + 8 * q + 4 * h;
          const int oy = oy0 + (pp >> g.lw), ox = ox0 + (pp & (TW - 1));
          if (oy >= H || ox >= W) continue;  // (W % 4 == 0: four positions are inside or outside as a whole)
          epilogue_store4<ACT>(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3], bm,
                               residual, y, chan + (long long)oy * W + ox);
        }
    }
  };
  with_act(act, epilogue);  // wave-uniform: one epilogue body per activation, the GEMM shared
}

// the shape rules of the entry (MTR_E_SHAPE: the caller takes another path); fills g
static int conv3x3_split_shape(C3sGeo& g, long long B, int Cin, int Cout, int H, int W) {
  if (B < 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  // 16-byte groups of 8 split input channels; 16-byte groups of four columns of x, y and the residual
  if (Cin % 8 || W % 4) return MTR_E_SHAPE;
  const long long Cp = (Cin + kC3sCK - 1) / kC3sCK * kC3sCK;
  const long long lim = 0x7fffffffLL, n = B > 0 ? B : 1;
  if (n * Cin * H * W > lim || n * Cout * H * W > lim || 27LL * Cout * Cp > lim) return MTR_E_SHAPE;
  g = C3sGeo{};
  g.Cin = Cin, g.Cp = (int)Cp, g.M = Cout, g.H = H, g.W = W;
  g.lw = W > 16 ? 5 : 4;
  const int TW = 1 << g.lw, TH = kC3sBN >> g.lw;
  g.LW = TW == 32 ? 40 : 32, g.HH = TH + 2, g.GW = (TW + 8) / 4;
  g.piece = g.HH * g.LW * kC3sCK * 2;
  g.cfg = Cout <= 32 ? 0 : Cout <= 64 ? 1 : (Cout + 95) / 96 * 96 < (Cout + 127) / 128 * 128 ? 3 : 2;
  const int mb = g.cfg == 3 ? 96 : 32 << g.cfg;
  const long long m_blocks = (Cout + mb - 1) / mb, xt = (W + TW - 1) / TW, yt = (H + TH - 1) / TH;
  const long long blocks = n * yt * xt * m_blocks;
  if (blocks > lim) return MTR_E_SHAPE;  // the grid
  g.m_blocks = (unsigned)m_blocks, g.xt = (unsigned)xt, g.yt = (unsigned)yt;
  g.blocks = (unsigned)(B * yt * xt * m_blocks);
  g.div_mb = make_fastdiv(g.m_blocks), g.div_xt = make_fastdiv(g.xt), g.div_yt = make_fastdiv(g.yt);
  g.div_gw = make_fastdiv((unsigned)g.GW);
  return MTR_OK;
}
static_assert(18 * 32 <= kC3sMaxPos && 10 * 40 <= kC3sMaxPos, "the halo images of both tile shapes");
static_assert(10 * 10 * 4 <= 256 * kC3sXV && 18 * 6 * 4 <= 256 * kC3sXV, "the loader units of both tile shapes");

}  // namespace mtr

extern "C" size_t mtr_conv3x3_split_lds_bytes(long long B, int Cin, int Cout, int H, int W) {
  mtr::C3sGeo g;
  if (B <= 0 || mtr::conv3x3_split_shape(g, B, Cin, Cout, H, W) != MTR_OK) return 0;
  return 2 * 3 * (size_t)g.piece;
}

extern "C" int mtr_conv3x3_bias_act_split(const void* x, const void* w_split, const float* bias, const void* residual,
                                          int act_code, long long B, int Cin, int Cout, int H, int W, void* y,
                                          mtr_stream_t stream) {
  using namespace mtr;
  C3sGeo g;
  const size_t plane = (size_t)H * W;
  const int e = dense3x3_check(x, w_split, bias, residual, y, act_code, B, Cin, Cout, plane, plane,
                               [&] { return conv3x3_split_shape(g, B, Cin, Cout, H, W); });
  if (e != MTR_OK) return e;
  if (B == 0) return MTR_OK;  // nothing to do
  const size_t lds = 2 * 3 * (size_t)g.piece;   // above the 64 KiB a kernel gets by default
  const auto go = [&](auto kern) -> int {
    const int e = allow_dynamic_lds((const void*)kern, kC3sMaxLds);
    if (e != MTR_OK) return e;
    MTR_CLEAR_STALE();
    hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(256), lds, (hipStream_t)stream, (const float*)x, (const uint4*)w_split,
                       bias, (const float*)residual, (float*)y, g, act_code);
    MTR_CHECK_LAUNCH();
    return MTR_OK;
  };
  if (g.cfg == 0) return go(conv3x3_split_kernel<1, 4, 1, 2>);
  if (g.cfg == 1) return go(conv3x3_split_kernel<2, 2, 1, 4>);
  if (g.cfg == 3) return go(conv3x3_split_kernel<1, 4, 3, 2>);
  return go(conv3x3_split_kernel<2, 2, 2, 4>);
}
