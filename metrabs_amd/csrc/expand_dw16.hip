// K25h: the function of expand_dw16.h on the planes K11 runs on its stride-1 BLOCK kernel
// (depthwise3x3_s1_block_kernel, depthwise.hip), up to 256 positions, with the squeeze-excite mean.
//
// Not part of the reference's hot path (like K10 - K16h): the stride-1 MBConv blocks of the backbone's 16-bit
// inference copy (backbones.fold_batchnorm(dtype=f16 / bf16, fuse_expand_depthwise=True)).  A depthwise convolution is
// per channel, so a workgroup that owns a slice of CM expanded channels of one image over the WHOLE plane needs nothing
// from another workgroup:
//
//   phase 1  edw_gemm_plane over the 1, 2, 4 or 8 position tiles of the plane (EdwTiles); the (row, column) of a
//            position by a shift.
//   between  the slice's image [c][H + 2][W + 8] (image column j at index j + 4: 8-byte stores and loads).
//   phase 2  one lane per (channel, 4 x 4 block of outputs), lanes indexed local = (ty << tw_log2) | tx inside an
//            aligned group of lp = H W / 16 lanes as in depthwise3x3_s1_block_kernel: the 6 x 6 window from LDS, the
//            accumulator started at the bias, nine fmaf in (ky, kx) order, settled(activate()), one rounding, four
//            8-byte row stores; the mean from the 16 rounded outputs in (row, column) order, the lp lanes combined by
//            __shfl_xor with m = lp / 2 .. 1, times 1.0f / (H * W).
//
// The workgroup-to-image mapping is edw_image_chunk's (`mapping` 0: plain, 1: one image's chunks on one XCD).
#include "expand_dw16.h"

namespace mtr {

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
  static_assert(EdwXTile<BN>::NU == 1, "one loader unit per thread at most");
  extern __shared__ __attribute__((aligned(16))) unsigned short edw_lds[];
  unsigned short* xs = edw_lds;  // phase 1: [2][BN * LDK], the X^T image of a k-tile
  unsigned short* ms = edw_lds;  // afterwards: [CM][H + 2][LW], the slice of the expanded activation

  int b, chunk;
  edw_image_chunk(g.xcd_map, g.chunks, b, chunk);
  if (b >= B) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int r = lane & 31, h = lane >> 5;
  const int M = g.Cmid, K = g.Cin, HW = g.HW;
  const int m0 = chunk * CM;

  // ---- phase 1; this lane's channels: cl + 32 i of the slice
  const int cl = wm * (32 * FM) + r;
  const EdwPlaneTiles tiles = {wn * (32 * FN)};
  edw_f32x16 acc[FM][FN];
  edw_gemm_plane<Hh, BN>(acc, xs, x + (long long)b * K * HW, w1, m0 + cl, M, K, HW, tid, tiles);

  // ---- the X^T buffers are free: the slice's image (CM % 64 == 0, LW % 4 == 0: whole 16-byte groups)
  edw_zero_image(ms, CM * g.plane, tid);
  __syncthreads();
  const int w_log2 = g.tw_log2 + 2;
  edw_store_expanded<Hh>(
      acc, act1, bias1, m0, M, cl, h, tiles, 0, 0, HW,
      [&](int p, int& row, int& col) { row = p >> w_log2, col = p & (g.W - 1); },
      EdwImage{ms, g.plane, g.LW, -1, kEdwColPad});
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

// the shape rules of the entry (MTR_E_SHAPE: the caller keeps the two-kernel chain); fills g
static int expand_dw16_shape(EdwGeo& g, long long B, int Cin, int Cmid, int H, int W) {
  if (B < 0 || Cin <= 0 || Cmid <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (Cin % 8 || H % 4 || W % 4) return MTR_E_SHAPE;  // 16-byte groups of k; whole 4 x 4 blocks
  // the planes K11 runs on its stride-1 block kernel, up to 256 positions
  if (!edw_k11_block_plane(H, W, 4)) return MTR_E_SHAPE;
  if (B * Cmid >= (1LL << 24)) return MTR_E_SHAPE;  // (past this K11 takes its generic kernel: other bits)
  const int HW = H * W;
  if ((long long)Cin * HW > 0x7fffffffLL || (long long)Cmid * 9 > 0x7fffffffLL) return MTR_E_SHAPE;
  g = EdwGeo{};
  g.Cin = Cin, g.Cmid = Cmid, g.H = H, g.W = W, g.HW = HW;
  g.tw_log2 = edw_ilog2_exact(W / 4), g.lp_log2 = g.tw_log2 + edw_ilog2_exact(H / 4);
  g.LW = W + 2 * kEdwColPad, g.plane = (H + 2) * g.LW;
  g.xcd_map = 1;
  g.inv_hw = 1.0f / (float)(H * W);
  return MTR_OK;
}

template <int DT, int NPT>
static int launch_expand_dw16_cfg(const EdwArgs& a, EdwGeo g) {
  using Tl = EdwTiles<NPT>;
  g.chunks = (g.Cmid + Tl::CM - 1) / Tl::CM;
  auto kern = expand_dw16_kernel<DT, NPT>;
  return edw_launch((const void*)kern, a, (size_t)2 * Tl::BN * kEdwLDK * sizeof(unsigned short),
                    (size_t)Tl::CM * g.plane * sizeof(unsigned short),
                    (g.xcd_map ? (a.B + 7) / 8 * 8 : a.B) * g.chunks, [&](dim3 grid, size_t lds) {
                      hipLaunchKernelGGL(kern, grid, dim3(256), lds, a.stream, (const unsigned short*)a.x,
                                         (const unsigned short*)a.w1, a.bias1, a.wd, a.bias2, (unsigned short*)a.y,
                                         a.row_mean, g, (int)a.B, a.act1, a.act2);
                    });
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
  const mtr::EdwArgs a = {x, w1, bias1, w_dw, bias_dw, y, row_mean, act1_code, act2_code, B, (hipStream_t)stream};
  mtr::EdwGeo g;
  const int e = mtr::edw_check(a, dtype, Cin, Cmid, mapping, [&](int& hw_in, int& hw_out) {
    const int es = mtr::expand_dw16_shape(g, B, Cin, Cmid, H, W);
    if (es == MTR_OK) hw_in = hw_out = g.HW;
    return es;
  });
  if (e != MTR_OK) return e;
  if (B == 0) return MTR_OK;
  if (mapping >= 0) g.xcd_map = mapping;
  return dtype == MTR_F16 ? mtr::launch_expand_dw16<MTR_F16>(a, g) : mtr::launch_expand_dw16<MTR_BF16>(a, g);
}

extern "C" int mtr_expand_dw16(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                               const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin, int Cmid,
                               int H, int W, void* y, float* row_mean, mtr_stream_t stream) {
  return mtr_expand_dw16_opts(x, dtype, w1, bias1, act1_code, w_dw, bias_dw, act2_code, B, Cin, Cmid, H, W, y,
                              row_mean, stream, -1);
}
