// K26h: the function of expand_dw16.h, with the mean, on the planes K25h (expand_dw16.hip) refuses because K11 runs
// them on its GENERIC kernel (depthwise3x3_kernel): 24x24 and 12x12 of the EfficientNetV2 family at 384 px, and every
// other plane up to 576 positions whose W / 4 or H / 4 is no power of two.  The bits of K13h followed by K11's generic
// kernel are also the bits of K13h + K18 (depthwise3x3_blocks.hip).
//
// Not part of the reference's hot path (like K10 - K25h): backbones.fold_batchnorm(dtype=f16 / bf16,
// fuse_expand_depthwise_planes=True).  A workgroup of four waves owns CM expanded channels of one image over the whole
// plane:
//
//   phase 1  edw_gemm_plane over ceil(H W / 32) position tiles of any count: FN per wave, WN waves along the positions
//            (the tiles past the plane compute zeros and store nothing); a loader thread owns up to three units.  The
//            (row, column) of a position comes from a division by W.
//   between  the slice's image [c][H + 2][W + 8] (image column j at index j + 4).
//   phase 2  depthwise3x3_kernel's mapping and arithmetic: lpp = min(64, next power of two >= groups) lanes per
//            channel (groups = H W / 4 groups of four horizontally adjacent outputs), 64 / lpp channels per wave, lane
//            `sub` walks the groups sub, sub + 64, ...  Per output the accumulator starts at 0, nine fmaf with ky outer
//            and kx inner, acc + bias, activate, settled(), one rounding through K11's element types.  The mean: each
//            group summed left to right from 0.0f, the lane's groups added in ascending order from 0.0f, the xor
//            butterfly lpp / 2 .. 1, times 1.0f / (float)(H W).  No LDS for partial sums.
//
// The workgroup-to-image mapping is edw_image_chunk's, as K25h's.
#include "expand_dw16.h"

namespace mtr {

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
  using Hh = EdwBits<DT>;
  using T = typename Hh::T;
  using Tl = EdpTiles<FN, WN>;
  constexpr int WM = Tl::WM, CM = Tl::CM, BN = Tl::BN;
  extern __shared__ __attribute__((aligned(16))) unsigned short edp_lds[];
  unsigned short* xs = edp_lds;  // phase 1: [2][BN * LDK], the X^T image of a k-tile
  unsigned short* ms = edp_lds;  // afterwards: [CM][H + 2][LW], the slice of the expanded activation

  int b, chunk;
  edw_image_chunk(g.xcd_map, g.chunks, b, chunk);
  if (b >= B) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int r = lane & 31, h = lane >> 5;
  const int M = g.Cmid, K = g.Cin, HW = g.HW;
  const int m0 = chunk * CM;

  // ---- phase 1; this lane's channel: cl of the slice
  const int cl = wm * 32 + r;
  const EdwPlaneTiles tiles = {wn * (32 * FN)};
  edw_f32x16 acc[1][FN];
  edw_gemm_plane<Hh, BN>(acc, xs, x + (long long)b * K * HW, w1, m0 + cl, M, K, HW, tid, tiles);

  // ---- the X^T buffers are free: the slice's image (CM % 64 == 0, LW % 4 == 0: whole 16-byte groups)
  edw_zero_image(ms, CM * g.plane, tid);
  __syncthreads();
  edw_store_expanded<Hh>(
      acc, act1, bias1, m0, M, cl, h, tiles, 0, 0, HW,
      [&](int p, int& row, int& col) { row = (int)fastdiv((unsigned)p, g.d_w), col = p - row * g.W; },
      EdwImage{ms, g.plane, g.LW, -1, kEdwColPad});
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
          const V4 mid4 = *reinterpret_cast<const V4*>(row + kEdwColPad);
          float in[6];
          in[0] = to_f32(__builtin_bit_cast(T, row[kEdwColPad - 1]));
#pragma unroll
          for (int j = 0; j < 4; ++j) in[1 + j] = to_f32(mid4.v[j]);
          in[5] = to_f32(__builtin_bit_cast(T, row[kEdwColPad + 4]));
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

// the shape rules of the entry (MTR_E_SHAPE: the caller keeps the two-kernel chain); fills g
static int expand_dw16_planes_shape(EdpGeo& g, long long B, int Cin, int Cmid, int H, int W) {
  if (B < 0 || Cin <= 0 || Cmid <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (Cin % 8 || W % 4) return MTR_E_SHAPE;  // 16-byte groups of k; whole groups of four outputs
  if (H > 32 || W > 32 || H * W > 576 || (H * W) % 8) return MTR_E_SHAPE;  // 16-byte groups of positions
  if (edw_k11_block_plane(H, W)) return MTR_E_SHAPE;  // (K11's block kernel: other bits; K25h's planes among them)
  if (B * Cmid >= (1LL << 30)) return MTR_E_SHAPE;  // (the generic kernel's own limit)
  const int HW = H * W;
  if ((long long)Cin * HW > 0x7fffffffLL || (long long)Cmid * 9 > 0x7fffffffLL) return MTR_E_SHAPE;
  g = EdpGeo{};
  g.Cin = Cin, g.Cmid = Cmid, g.H = H, g.W = W, g.HW = HW;
  g.LW = W + 2 * kEdwColPad, g.plane = (H + 2) * g.LW;
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

template <int DT, int FN, int WN>
static int launch_expand_dw16_planes_cfg(const EdwArgs& a, EdpGeo g) {
  using Tl = EdpTiles<FN, WN>;
  g.chunks = (g.Cmid + Tl::CM - 1) / Tl::CM;
  auto kern = expand_dw16_planes_kernel<DT, FN, WN>;
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
static int launch_expand_dw16_planes(const EdwArgs& a, const EdpGeo& g) {
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
  mtr::EdwArgs a = {};
  a.B = B;
  const int n = mtr::launch_expand_dw16_planes<MTR_F16>(a, g);
  return n > 0 ? (size_t)n : 0;
}

extern "C" int mtr_expand_dw16_planes_opts(const void* x, int dtype, const void* w1, const float* bias1,
                                           int act1_code, const float* w_dw, const float* bias_dw, int act2_code,
                                           long long B, int Cin, int Cmid, int H, int W, void* y, float* row_mean,
                                           mtr_stream_t stream, int mapping) {
  const mtr::EdwArgs a = {x, w1, bias1, w_dw, bias_dw, y, row_mean, act1_code, act2_code, B, (hipStream_t)stream};
  mtr::EdpGeo g;
  const int e = mtr::edw_check(a, dtype, Cin, Cmid, mapping, [&](int& hw_in, int& hw_out) {
    const int es = mtr::expand_dw16_planes_shape(g, B, Cin, Cmid, H, W);
    if (es == MTR_OK) hw_in = hw_out = g.HW;
    return es;
  });
  if (e != MTR_OK) return e;
  if (B == 0) return MTR_OK;
  if (mapping >= 0) g.xcd_map = mapping;
  return dtype == MTR_F16 ? mtr::launch_expand_dw16_planes<MTR_F16>(a, g)
                          : mtr::launch_expand_dw16_planes<MTR_BF16>(a, g);
}

extern "C" int mtr_expand_dw16_planes(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                                      const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin,
                                      int Cmid, int H, int W, void* y, float* row_mean, mtr_stream_t stream) {
  return mtr_expand_dw16_planes_opts(x, dtype, w1, bias1, act1_code, w_dw, bias_dw, act2_code, B, Cin, Cmid, H, W, y,
                                     row_mean, stream, -1);
}
