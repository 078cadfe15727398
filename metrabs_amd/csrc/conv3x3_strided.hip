// K22: a dense 3x3 convolution (stride 2, padding 1, groups 1) of f32 NCHW tensors as an implicit GEMM on the
// f32-input MFMA, with the K10 epilogue folded in.
//
// Not part of the reference's hot path (like K10 - K20): the dense 3x3 stride-2 layers of the f32 inference copy
// (backbones.fold_batchnorm(fused_epilogue=True, strided3x3=True)) -- the first blocks of EfficientNetV2's FusedMBConv
// stages 2 and 3, the stride-2 `a` layers of ResNet-18's BasicBlocks.  PyTorch-ROCm runs each as a MIOpen direct
// convolution, then K10.  Here, in one launch, for H and W even (OH = H / 2, OW = W / 2):
//
//   y[b, m, oy, ox] = act(bias[m] + sum_{ci, ky, kx} w[m, ci, ky, kx] * x[b, ci, 2 oy + ky - 1, 2 ox + kx - 1])
//                     (+ residual[b, m, oy, ox])
//
// THE ARITHMETIC.  Every output element is ONE chain of 9 Cin fused multiply-adds that starts from 0:
//
//   s = 0
//   for c4 = 0, 4, 8, ... < Cin:            (the chunks: four input channels)
//     for ky = 0, 1, 2:  for kx = 0, 1, 2:  (the taps, rows first)
//       for ci = c4, c4 + 1, c4 + 2, c4 + 3:
//         s = fmaf(x[b, ci, 2 oy + ky - 1, 2 ox + kx - 1], w[m, ci, ky, kx], s)      (x = 0 outside the image)
//
// -- one v_mfma_f32_16x16x4_f32 per (c4, ky, kx), whose four k are the four ci, and an MFMA is bitwise a k-ordered
// fmaf chain.  Then "+ bias", the activation, "+ residual": K10's order (common.h: epilogue_store4).  No split-K, no
// atomics, no workspace.  Nothing in the chain depends on the batch index, on where a tile lies or on which tile
// shape the launch uses: the same inputs give the same bits on every call and graph replay.
//
// Computed transposed, as K20 does: positions on the MFMA's A rows, output channels on its B columns.  A position
// fragment is 16 consecutive ox of one output row; register e of an accumulator is then position 4 (lane >> 4) + e of
// channel lane & 15: four consecutive ox of one channel, one 16-byte store, the epilogue in registers.
//
// One workgroup of four waves takes 8 position fragments of one image -- TR output rows x TF fragments, TF = 4, 2 or
// 1 and TR = 8 / TF, whichever leaves the fewest empty fragments on the row: the only thing that differs between the
// three instantiations is where a fragment lies -- and a block of up to 128 output channels (M <= 128: all of them;
// above: ceil(M / 128) equal blocks, the blocks of one tile next to each other in the grid so that the second reads x
// from L2).  Wave w owns fragments 2 w and 2 w + 1 for all channel fragments of the block: 2 x 8 accumulators, 64
// registers.  The workgroup walks Cin in chunks of 4:
//   * every thread loads its share of the NEXT chunk -- three 16-byte groups of the input halo ((2 TR + 1) rows x
//     (32 TF + 1) columns of 4 planes; only the top row and the left column of an even plane can be padding), one
//     left-column element, five 16-byte groups of the chunk's weight block -- into registers before this chunk's
//     MFMAs.  Every load is unconditional: an element outside the image is read from a valid address and replaced by
//     0 on the way into LDS, and behind the last chunk the last chunk is requested again and dropped;
//   * the halo is de-interleaved by column parity on the way into LDS: a row of the image is [E: 16 TF | . | O: 16 TF
//     + 1], E[c] = column 2 (ox0 + c), O[c] = column 2 (ox0 + c) - 1.  Tap kx = 1 reads E[c], taps kx = 0, 2 read O[c]
//     and O[c + 1]: unit stride across the 16 lanes of a fragment.  The four ci planes lie PS floats apart, PS = 16
//     mod 32, so the four k of a fragment read sit on different halves of the 32 ds_read_b32 banks: conflict-free;
//   * the weight arrives packed [Cin / 4][Cout][ky][kx][ci % 4] (kernels.pack_conv3x3_strided_weight), so a chunk's
//     block is one contiguous run of 36 floats per channel; it goes to LDS as [m][38]: lane (c, kq) of a B fragment
//     reads word 38 c + 4 tap + kq, and 38 c mod 32 runs over the 16 even banks: conflict-free too;
//   * per channel fragment: 9 B reads and 18 MFMAs on two independent accumulators (the 18 A values of the chunk are
//     read once, in front).
#include "common.h"

namespace mtr {

typedef float s2_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kS2CK = 4;     // input channels per chunk: the four k of one MFMA
constexpr int kS2MB = 128;   // output channels per workgroup at most (8 channel fragments)
constexpr int kS2NCF = kS2MB / 16;
constexpr int kS2LW = 38;    // floats between the [m] rows of the weight image: 36 + 2, 38 c mod 32 distinct for c < 16
constexpr int kS2WV = (kS2MB * 9 + 255) / 256;  // 16-byte weight groups per thread and chunk

template <int TFL>
struct S2Tile {
  static constexpr int TF = 1 << TFL;        // position fragments per output row of the tile
  static constexpr int TR = 8 >> TFL;        // output rows of the tile
  static constexpr int NR = 2 * TR + 1;      // input rows of the halo
  static constexpr int Q = 8 * TF;           // 16-byte groups per input row (columns 2 ox0 ... 2 ox0 + 32 TF - 1)
  static constexpr int RS = 32 * TF + 2;     // floats per row of the image: E at 0, O[c] at 16 TF + 1 + c
  static constexpr int PS = NR * RS + ((16 - (NR * RS) % 32) + 32) % 32;  // floats per plane, = 16 mod 32
  static constexpr int NIT = kS2CK * NR * Q; // 16-byte groups of the halo per chunk
  static constexpr int XV = (NIT + 255) / 256;
  static_assert(PS % 32 == 16 && RS % 2 == 0 && kS2CK * NR <= 256, "bank spacing, 8-byte rows, one left element each");
};
constexpr int kS2XsFloats = kS2CK * 656;  // the largest of the three images (TF = 4: 4 planes of 656 floats)
static_assert(kS2CK * S2Tile<0>::PS <= kS2XsFloats && kS2CK * S2Tile<1>::PS <= kS2XsFloats &&
              kS2CK * S2Tile<2>::PS <= kS2XsFloats, "the halo image");
constexpr size_t kS2LdsBytes = (size_t)(kS2XsFloats + kS2MB * kS2LW) * sizeof(float);

// the geometry of one launch, computed on the host (conv3x3s2_shape)
struct S2Geo {
  int Cin, M, H, W, OH, OW;
  int tfl;                       // log2 TF
  int mb_size;                   // channels per channel block (a multiple of 16, <= 128)
  unsigned m_blocks, xt, rt;     // channel blocks, tiles per row, tiles per column
  unsigned blocks;               // B rt xt m_blocks
  FastDiv div_mb, div_xt, div_rt;
};

template <int TFL>
__global__ __launch_bounds__(256) void conv3x3s2_kernel(
    const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias,
    const float* __restrict__ residual, float* __restrict__ y, S2Geo g, int act) {
  using T = S2Tile<TFL>;
  __shared__ __align__(16) float xs[kS2XsFloats];
  __shared__ __align__(16) float ws[kS2MB * kS2LW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int Cin = g.Cin, M = g.M, H = g.H, W = g.W, OH = g.OH, OW = g.OW;
  const int plane = H * W;

  // ---- the workgroup's tile: channel block fastest, then the tile of the row, the row of tiles, the image
  unsigned id = blockIdx.x;
  unsigned q = fastdiv(id, g.div_mb);
  const int mb = (int)(id - q * g.m_blocks);
  id = q, q = fastdiv(id, g.div_xt);
  const int ox0 = (int)(id - q * g.xt) * 16 * T::TF;
  id = q, q = fastdiv(id, g.div_rt);
  const int oy0 = (int)(id - q * g.rt) * T::TR;
  const long long b = q;
  const int m0 = mb * g.mb_size;
  const int Mb = min(g.mb_size, M - m0);       // channels of this block (>= 1)
  const int ncf = (Mb + 15) >> 4;              // its channel fragments
  const int nwv = Mb * 9;                      // 16-byte groups of a chunk's weight block

  // ---- the loader's share of a chunk (the same for every chunk)
  const float* xb = x + b * Cin * plane;
  int goff[T::XV], loff[T::XV];
  bool inimg[T::XV], mine[T::XV];
#pragma unroll
  for (int j = 0; j < T::XV; ++j) {
    const int idx = tid + 256 * j;
    const int qq = idx % T::Q, rr = (idx / T::Q) % T::NR, pl = idx / (T::Q * T::NR);
    const int iy = 2 * oy0 - 1 + rr, ix = 2 * ox0 + 4 * qq;
    mine[j] = idx < T::NIT;
    inimg[j] = mine[j] && iy >= 0 && iy < H && ix < W;  // (W % 8 == 0: a group is inside or outside as a whole)
    goff[j] = inimg[j] ? pl * plane + iy * W + ix : 0;
    loff[j] = pl * T::PS + rr * T::RS + 2 * qq;
  }
  // the left column of the halo, O[0]: one element per (plane, row)
  const bool lmine = tid < kS2CK * T::NR;
  const int lpl = tid / T::NR, lrr = tid % T::NR, liy = 2 * oy0 - 1 + lrr;
  const bool linimg = lmine && ox0 > 0 && liy >= 0 && liy < H;
  const int lgoff = linimg ? lpl * plane + liy * W + 2 * ox0 - 1 : 0;
  const int lloff = lpl * T::PS + lrr * T::RS + 16 * T::TF + 1;

  float4 xv[T::XV], wv[kS2WV];
  float xl;
  auto load_chunk = [&](int c0) {
    const float* xc = xb + c0 * plane;
#pragma unroll
    for (int j = 0; j < T::XV; ++j) xv[j] = *reinterpret_cast<const float4*>(xc + goff[j]);
    xl = xc[lgoff];
    const float* wc = wp + ((long long)(c0 >> 2) * M + m0) * 36;
#pragma unroll
    for (int j = 0; j < kS2WV; ++j)
      wv[j] = *reinterpret_cast<const float4*>(wc + 4 * min(tid + 256 * j, nwv - 1));
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int j = 0; j < T::XV; ++j) {
      if (!mine[j]) continue;
      const float4 v = inimg[j] ? xv[j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      // columns 4 q, 4 q + 2 are E[2 q], E[2 q + 1]; columns 4 q + 1, 4 q + 3 are O[2 q + 1], O[2 q + 2]
      *reinterpret_cast<float2*>(xs + loff[j]) = make_float2(v.x, v.z);
      *reinterpret_cast<float2*>(xs + loff[j] + 16 * T::TF + 2) = make_float2(v.y, v.w);
    }
    if (lmine) xs[lloff] = linimg ? xl : 0.0f;
#pragma unroll
    for (int j = 0; j < kS2WV; ++j) {
      const int idx = tid + 256 * j;
      if (idx >= nwv) continue;
      const int mr = idx / 9, t = idx - 9 * mr;
      float* dst = ws + mr * kS2LW + 4 * t;
      *reinterpret_cast<float2*>(dst) = make_float2(wv[j].x, wv[j].y);
      *reinterpret_cast<float2*>(dst + 2) = make_float2(wv[j].z, wv[j].w);
    }
  };

  s2_f32x4 acc[2][kS2NCF];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int cf = 0; cf < kS2NCF; ++cf)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][cf][e] = 0.0f;

  // fragment addresses: lane (p, kq) = (lane & 15, lane >> 4) reads plane / ci kq of position p (A), of channel p (B)
  const int l15 = lane & 15, kq = lane >> 4;
  const int f0 = 2 * wave, f1 = 2 * wave + 1;
  const int fr0 = f0 >> TFL, fx0 = f0 & (T::TF - 1), fr1 = f1 >> TFL, fx1 = f1 & (T::TF - 1);
  const float* afrag0 = xs + kq * T::PS + 2 * fr0 * T::RS + 16 * fx0 + l15;
  const float* afrag1 = xs + kq * T::PS + 2 * fr1 * T::RS + 16 * fx1 + l15;
  const float* bfrag = ws + l15 * kS2LW + kq;

  load_chunk(0);
  for (int c0 = 0; c0 < Cin; c0 += kS2CK) {
    store_chunk();
    __syncthreads();
    load_chunk(min(c0 + kS2CK, Cin - kS2CK));  // in flight under this chunk's MFMAs (the last one again at the end)
    float a0[9], a1[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int off = ky * T::RS + (kx == 1 ? 0 : kx == 0 ? 16 * T::TF + 1 : 16 * T::TF + 2);
        a0[3 * ky + kx] = afrag0[off];
        a1[3 * ky + kx] = afrag1[off];
      }
#pragma unroll
    for (int cf = 0; cf < kS2NCF; ++cf) {
      if (cf < ncf) {  // wave-uniform
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const float bv = bfrag[cf * 16 * kS2LW + 4 * t];
          acc[0][cf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[t], bv, acc[0][cf], 0, 0, 0);
          acc[1][cf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[t], bv, acc[1][cf], 0, 0, 0);
        }
      }
    }
    __syncthreads();  // every wave has read this chunk's fragments: the images are rewritten
  }

  // ---- the epilogue: register e of acc[i][cf] is channel m0 + 16 cf + l15 at ox = ox0 + 16 fx_i + 4 kq + e
  const int mlast = m0 + Mb;
  const long long oplane = (long long)OH * OW;
  auto epilogue = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int oy = oy0 + (i ? fr1 : fr0), ox = ox0 + 16 * (i ? fx1 : fx0) + 4 * kq;
      if (oy >= OH || ox >= OW) continue;  // (OW % 4 == 0: four positions are inside or outside as a whole)
#pragma unroll
      for (int cf = 0; cf < kS2NCF; ++cf) {
        const int m = m0 + 16 * cf + l15;
        if (m >= mlast) continue;
        const long long off = (b * M + m) * oplane + (long long)oy * OW + ox;
        epilogue_store4<ACT>(acc[i][cf][0], acc[i][cf][1], acc[i][cf][2], acc[i][cf][3], bias[m], residual, y, off);
      }
    }
  };
  with_act(act, epilogue);  // wave-uniform: one epilogue body per activation, the GEMM shared
}

// the shape rules of the entry (MTR_E_SHAPE: the caller takes the library path); fills g for B > 0
static int conv3x3s2_shape(S2Geo& g, long long B, int Cin, int Cout, int H, int W) {
  if (B < 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  // chunks of four ci; even planes (only the top row and the left column are padding); 16-byte groups of four ox
  if (Cin % 4 || H % 2 || W % 2 || (W / 2) % 4) return MTR_E_SHAPE;
  const int OH = H / 2, OW = W / 2;
  if ((long long)Cin * H * W > 0x7fffffffLL || (long long)Cout * OH * OW > 0x7fffffffLL ||
      (long long)Cin * Cout * 9 > 0x7fffffffLL)
    return MTR_E_SHAPE;
  // the row's fragments in tiles of 4, 2 or 1: the widest tile among those that leave the fewest empty fragments
  const int fx = (OW + 15) / 16;
  int tfl = 0;
  for (int t = 1; t <= 2; ++t)
    if ((fx + (1 << t) - 1) / (1 << t) * (1 << t) <= (fx + (1 << tfl) - 1) / (1 << tfl) * (1 << tfl)) tfl = t;
  const int tf = 1 << tfl, tr = 8 >> tfl;
  const long long m_blocks = (Cout + kS2MB - 1) / kS2MB;
  const long long xt = (fx + tf - 1) / tf, rt = (OH + tr - 1) / tr;
  const long long blocks = B * rt * xt * m_blocks;
  if (blocks > 0x7fffffffLL) return MTR_E_SHAPE;  // the grid
  g = S2Geo{};
  g.Cin = Cin, g.M = Cout, g.H = H, g.W = W, g.OH = OH, g.OW = OW, g.tfl = tfl;
  g.mb_size = (int)(((Cout + m_blocks - 1) / m_blocks + 15) / 16 * 16);
  g.m_blocks = (unsigned)((Cout + g.mb_size - 1) / g.mb_size);
  g.xt = (unsigned)xt, g.rt = (unsigned)rt;
  g.blocks = (unsigned)(B * rt * xt * g.m_blocks);
  g.div_mb = make_fastdiv(g.m_blocks), g.div_xt = make_fastdiv(g.xt), g.div_rt = make_fastdiv(g.rt);
  return MTR_OK;
}

}  // namespace mtr

extern "C" size_t mtr_conv3x3s2_lds_bytes(long long B, int Cin, int Cout, int H, int W) {
  mtr::S2Geo g;
  if (B <= 0 || mtr::conv3x3s2_shape(g, B, Cin, Cout, H, W) != MTR_OK) return 0;
  return mtr::kS2LdsBytes;
}

extern "C" int mtr_conv3x3s2_bias_act(const void* x, const float* w_packed, const float* bias, const void* residual,
                                      int act_code, long long B, int Cin, int Cout, int H, int W, void* y,
                                      mtr_stream_t stream) {
  using namespace mtr;
  S2Geo g;
  const int e = dense3x3_check(x, w_packed, bias, residual, y, act_code, B, Cin, Cout, (size_t)H * W,
                               (size_t)(H / 2) * (W / 2), [&] { return conv3x3s2_shape(g, B, Cin, Cout, H, W); });
  if (e != MTR_OK) return e;
  if (B == 0) return MTR_OK;  // nothing to do
  MTR_CLEAR_STALE();
  const dim3 grid(g.blocks), block(256);
  const float* xf = (const float*)x;
  const float* rf = (const float*)residual;
  float* yf = (float*)y;
  if (g.tfl == 2)
    hipLaunchKernelGGL(conv3x3s2_kernel<2>, grid, block, 0, (hipStream_t)stream, xf, w_packed, bias, rf, yf, g,
                       act_code);
  else if (g.tfl == 1)
    hipLaunchKernelGGL(conv3x3s2_kernel<1>, grid, block, 0, (hipStream_t)stream, xf, w_packed, bias, rf, yf, g,
                       act_code);
  else
    hipLaunchKernelGGL(conv3x3s2_kernel<0>, grid, block, 0, (hipStream_t)stream, xf, w_packed, bias, rf, yf, g,
                       act_code);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}
