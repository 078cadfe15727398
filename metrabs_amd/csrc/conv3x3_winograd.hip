// K19: a dense 3x3 convolution (stride 1, padding 1, groups 1) of f32 NCHW tensors as Winograd F(2x2, 3x3) on the
// f32-input MFMA, with the K10 epilogue folded in.
//
// Not part of the reference's hot path (like K10 - K18): the dense 3x3 stride-1 layers of the f32 inference copy
// (backbones.fold_batchnorm(fused_epilogue=True, winograd3x3=True)).  PyTorch-ROCm runs each as a MIOpen Winograd
// convolution, then K10.  Here, in one launch:
//
//   y[b, m, oy, ox] = act(bias[m] + sum_{ci, ky, kx} w[m, ci, ky, kx] * x[b, ci, oy + ky - 1, ox + kx - 1])
//                     (+ residual[b, m, oy, ox])
//
// evaluated per 2x2 output tile as  Y = A^T [ sum_ci U[xi, m, ci] * V[xi, ci, tile] ] A,  V = B^T d B  of the tile's
// 4x4 input patch d (zero outside the image), U = G g G^T handed in already transformed ([16][Cout][Cin], xi = 4 i + j).
// The standard matrices:  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1],  A^T = [1 1 1 0; 0 1 -1 -1].
//
// The tiles of the whole batch are numbered in raster order, n = (b, ty, tx).  One workgroup of four waves takes 32
// output channels x 64 consecutive tiles (no region geometry: maps of any even size, partial last workgroups and maps
// smaller than 64 tiles are the same code; 16 consecutive tiles of a 32-wide or wider map are 128 contiguous bytes of
// two output rows).  It walks Cin in chunks of 8:
//   * every thread loads the raw 4x4 patches of two (ci, tile) pairs and four 16-byte groups of U for the NEXT chunk
//     into registers before this chunk's MFMAs, so the loads fly under them; each element carries its own bounds
//     predicate, the padding ring and channels past Cin are zeros, and the k loop has no bounds tests;
//   * B^T d B is applied on the VALU, rows first, then columns, one fixed order of additions, into an LDS image of 16
//     [ci][tile] matrices (rows 80 floats apart); U's chunk is written beside it as 16 [ci][m] matrices (rows 48
//     floats apart): the four k of a fragment read are then 16 banks apart, every fragment ds_read_b32 conflict-free
//     (the U writes are not: lanes 2 m and 2 m + 1 write rows 4 x 48 floats apart, the same bank, two-way);
//   * wave w owns ALL 16 xi of its 32 channels x 16 tiles: 16 x 2 accumulators of v_mfma_f32_16x16x4_f32 (128
//     registers), A = U (channels on the rows), B = V (tiles on the columns), three fragment reads per two MFMAs.
//     The MFMA is a k-ordered fmaf chain, and the chunks follow one another, so every product sum runs over
//     ci = 0, 1, 2, ... in that one order.
// The C/D layout does not depend on the operands: the 16 xi of one (m, tile) sit in the same lane and register index,
// so A^T M A (M A over the columns first, then A^T over the rows) and the epilogue -- bias, activation, then the
// residual: K10's order -- run in registers.  A lane ends with 2x2 outputs of four channels; lanes 0 .. 15 of a quarter wave hold 16 consecutive
// tiles, so one 8-byte store instruction writes whole 128-byte row segments of four channels.
//
// Nothing depends on the batch index or on a tile configuration (there is one).  No atomics, no split-K, no
// workspace: the same inputs give the same bits on every call and graph replay.
#include "common.h"

namespace mtr {

typedef float wg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWgCK = 8;    // input channels per chunk (two k steps of the 16x16x4 MFMA)
constexpr int kWgBM = 32;   // output channels per workgroup (two 16-row MFMA tiles per wave)
constexpr int kWgBN = 64;   // Winograd tiles per workgroup (16 per wave)
constexpr int kWgLDV = 80;  // floats between the [xi][ci] rows of V: 64 tiles + 16, rows 16 banks apart
constexpr int kWgLDU = 48;  // floats between the [xi][ci] rows of U: 32 channels + 16
constexpr size_t kWgLdsBytes = (size_t)16 * kWgCK * (kWgLDV + kWgLDU) * sizeof(float);

// the geometry of one launch, computed on the host (conv3x3_winograd_shape)
struct WgGeo {
  int Cin, M, H, W;
  unsigned T, TX;        // tiles per image, tiles per row of tiles
  unsigned n_tiles;      // B T
  unsigned m_blocks;     // ceil(M / 32)
  FastDiv divT, divTX;
};

__global__ __launch_bounds__(256, 2) void conv3x3_winograd_kernel(
    const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ bias,
    const float* __restrict__ residual, float* __restrict__ y, WgGeo g, int act) {
  __shared__ float vs[16 * kWgCK * kWgLDV];
  __shared__ float us[16 * kWgCK * kWgLDU];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Cin = g.Cin, M = g.M, H = g.H, W = g.W;
  const unsigned mb = blockIdx.x % g.m_blocks, nb = blockIdx.x / g.m_blocks;
  const int m0 = (int)mb * kWgBM;
  const long long plane = (long long)H * W;

  // ---- the loader's tile: tile `lane` of the workgroup's 64, input channels wave and wave + 4 of each chunk
  const unsigned nl = nb * kWgBN + lane;
  unsigned mask = 0;        // bit 4 r + c: element (r, c) of the 4x4 patch lies inside the image
  long long xbase = 0;      // x index of the patch's element (0, 0) in channel 0 (may lie outside: never read then)
  if (nl < g.n_tiles) {
    const unsigned b = fastdiv(nl, g.divT), rem = nl - b * g.T;
    const unsigned ty = fastdiv(rem, g.divTX), tx = rem - ty * g.TX;
    const int iy0 = 2 * (int)ty - 1, ix0 = 2 * (int)tx - 1;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (iy0 + r >= 0 && iy0 + r < H && ix0 + c >= 0 && ix0 + c < W) mask |= 1u << (4 * r + c);
    xbase = (long long)b * Cin * plane + (long long)iy0 * W + ix0;
  }
  // U: group (xi = wave + 4 j, channel m0 + (lane >> 1), ci 4 (lane & 1) ... + 3 of the chunk)
  const int um = m0 + (lane >> 1), uq = 4 * (lane & 1);
  const bool um_ok = um < M;

  float raw[2][16];
  float4 uv[4];
  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ci = c0 + wave + 4 * j;
      const unsigned mk = ci < Cin ? mask : 0u;
      const long long base = xbase + (long long)ci * plane;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          raw[j][4 * r + c] = ((mk >> (4 * r + c)) & 1u) ? x[base + r * W + c] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int xi = wave + 4 * j;
      uv[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (um_ok && c0 + uq < Cin)  // (Cin % 4 == 0: the whole group is inside)
        uv[j] = *reinterpret_cast<const float4*>(u + ((long long)xi * M + um) * Cin + c0 + uq);
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float* d = raw[j];
      float t[16];
#pragma unroll
      for (int c = 0; c < 4; ++c) {  // B^T d
        t[c] = d[c] - d[8 + c];
        t[4 + c] = d[4 + c] + d[8 + c];
        t[8 + c] = d[8 + c] - d[4 + c];
        t[12 + c] = d[4 + c] - d[12 + c];
      }
      float* dst = vs + (wave + 4 * j) * kWgLDV + lane;
#pragma unroll
      for (int r = 0; r < 4; ++r) {  // (B^T d) B
        dst[(4 * r + 0) * kWgCK * kWgLDV] = t[4 * r] - t[4 * r + 2];
        dst[(4 * r + 1) * kWgCK * kWgLDV] = t[4 * r + 1] + t[4 * r + 2];
        dst[(4 * r + 2) * kWgCK * kWgLDV] = t[4 * r + 2] - t[4 * r + 1];
        dst[(4 * r + 3) * kWgCK * kWgLDV] = t[4 * r + 1] - t[4 * r + 3];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float* dst = us + ((wave + 4 * j) * kWgCK + uq) * kWgLDU + (lane >> 1);
      dst[0] = uv[j].x;
      dst[kWgLDU] = uv[j].y;
      dst[2 * kWgLDU] = uv[j].z;
      dst[3 * kWgLDU] = uv[j].w;
    }
  };

  wg_f32x4 acc[16][2];
#pragma unroll
  for (int xi = 0; xi < 16; ++xi)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[xi][i][e] = 0.0f;

  // fragment addresses: lane (c, kq) = (lane & 15, lane >> 4) reads k = 4 step + kq of channel / tile c
  const int l15 = lane & 15, kq = lane >> 4;
  const float* vfrag = vs + kq * kWgLDV + 16 * wave + l15;
  const float* ufrag = us + kq * kWgLDU + l15;

  load_chunk(0);
  for (int c0 = 0; c0 < Cin; c0 += kWgCK) {
    store_chunk();
    __syncthreads();
    if (c0 + kWgCK < Cin) load_chunk(c0 + kWgCK);  // in flight under this chunk's MFMAs
#pragma unroll
    for (int ks = 0; ks < kWgCK / 4; ++ks) {
#pragma unroll
      for (int xi = 0; xi < 16; ++xi) {
        const float bv = vfrag[(xi * kWgCK + 4 * ks) * kWgLDV];
        const float a0 = ufrag[(xi * kWgCK + 4 * ks) * kWgLDU], a1 = ufrag[(xi * kWgCK + 4 * ks) * kWgLDU + 16];
        acc[xi][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[xi][0], 0, 0, 0);
        acc[xi][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[xi][1], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave has read this chunk's fragments: the images are rewritten
  }

  // ---- A^T M A and the epilogue: register e of acc[xi][i] is channel m0 + 16 i + 4 kq + e of tile 16 wave + l15
  const unsigned no = nb * kWgBN + 16 * wave + l15;
  if (no >= g.n_tiles) return;
  const unsigned ob = fastdiv(no, g.divT), orem = no - ob * g.T;
  const unsigned oty = fastdiv(orem, g.divTX), otx = orem - oty * g.TX;
  const long long ybase = (long long)ob * M * plane + (long long)(2 * oty) * W + 2 * otx;
  auto epilogue = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + 16 * i + 4 * kq + e;
        if (m >= M) continue;
        float s[4][2];  // M A: columns
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          s[r][0] = (acc[4 * r][i][e] + acc[4 * r + 1][i][e]) + acc[4 * r + 2][i][e];
          s[r][1] = (acc[4 * r + 1][i][e] - acc[4 * r + 2][i][e]) - acc[4 * r + 3][i][e];
        }
        const float bm = bias[m];
        float o[2][2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {  // A^T (M A): rows
          o[0][c] = settled(activate<ACT>(((s[0][c] + s[1][c]) + s[2][c]) + bm));
          o[1][c] = settled(activate<ACT>(((s[1][c] - s[2][c]) - s[3][c]) + bm));
        }
        const long long at = ybase + (long long)m * plane;
        if (residual) {  // the block's skip connection, added after the activation (K10's order)
          const float2 r0 = *reinterpret_cast<const float2*>(residual + at);
          const float2 r1 = *reinterpret_cast<const float2*>(residual + at + W);
          o[0][0] += r0.x, o[0][1] += r0.y, o[1][0] += r1.x, o[1][1] += r1.y;
        }
        *reinterpret_cast<float2*>(y + at) = make_float2(o[0][0], o[0][1]);
        *reinterpret_cast<float2*>(y + at + W) = make_float2(o[1][0], o[1][1]);
      }
    }
  };
  with_act(act, epilogue);  // wave-uniform: one epilogue body per activation, the GEMM shared
}

// the shape rules of the entry (MTR_E_SHAPE: the caller takes the library path); fills g for B > 0
static int conv3x3_winograd_shape(WgGeo& g, long long B, int Cin, int Cout, int H, int W) {
  if (B < 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  // 2x2 output tiles; 8-byte groups of two columns of y and the residual at even columns; 16-byte groups of 4 ci of U
  if (H % 2 || W % 4 || Cin % 4) return MTR_E_SHAPE;
  if ((long long)Cin * H * W > 0x7fffffffLL || (long long)Cout * H * W > 0x7fffffffLL) return MTR_E_SHAPE;
  const long long T = (long long)(H / 2) * (W / 2), n_tiles = B * T;
  const long long m_blocks = (Cout + kWgBM - 1) / kWgBM;
  if (n_tiles > 0x7fffffffLL - kWgBN) return MTR_E_SHAPE;
  if (((n_tiles + kWgBN - 1) / kWgBN) * m_blocks > 0x7fffffffLL) return MTR_E_SHAPE;  // the grid
  g = WgGeo{};
  g.Cin = Cin, g.M = Cout, g.H = H, g.W = W;
  g.T = (unsigned)T, g.TX = (unsigned)(W / 2), g.n_tiles = (unsigned)n_tiles, g.m_blocks = (unsigned)m_blocks;
  g.divT = make_fastdiv(g.T), g.divTX = make_fastdiv(g.TX);
  return MTR_OK;
}

}  // namespace mtr

extern "C" size_t mtr_conv3x3_winograd_lds_bytes(long long B, int Cin, int Cout, int H, int W) {
  mtr::WgGeo g;
  if (B <= 0 || mtr::conv3x3_winograd_shape(g, B, Cin, Cout, H, W) != MTR_OK) return 0;
  return mtr::kWgLdsBytes;
}

extern "C" int mtr_conv3x3_winograd_bias_act(const void* x, const float* weight_u, const float* bias,
                                             const void* residual, int act, long long B, int Cin, int Cout, int H,
                                             int W, void* y, mtr_stream_t stream) {
  using namespace mtr;
  WgGeo g;
  const size_t plane = (size_t)H * W;
  const int e = dense3x3_check(x, weight_u, bias, residual, y, act, B, Cin, Cout, plane, plane,
                               [&] { return conv3x3_winograd_shape(g, B, Cin, Cout, H, W); });
  if (e != MTR_OK) return e;
  if (B == 0) return MTR_OK;  // nothing to do
  const unsigned blocks = (unsigned)(((long long)g.n_tiles + kWgBN - 1) / kWgBN) * g.m_blocks;
  MTR_CLEAR_STALE();
  hipLaunchKernelGGL(conv3x3_winograd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float*)x,
                     weight_u, bias, (const float*)residual, (float*)y, g, act);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}
