// K27h: the function of expand_dw16.h (stride 1 or 2, padding 1, no mean) on the LARGE planes K25h (expand_dw16.hip)
// and K26h (expand_dw16_planes.hip) refuse -- 64x64, 128x128 -> 64x64, 32x32 -> 16x16 of MobileNetV3's early blocks --
// where the expanded activation written by K13h and read straight back by K11 is nearly all of the chain's traffic.
// There is no squeeze-excite mean: without it an output needs only its 3x3 window of the expanded activation, so a
// workgroup owns a BAND of output rows instead of the whole plane and recomputes the halo rows of the expand.
//
// Not part of the reference's hot path (like K10 - K26h): backbones.fold_batchnorm(dtype=f16 / bf16,
// fuse_expand_depthwise_tiles=True).  The bits are those of conv1x1_16_kernel (K13h) followed by depthwise3x3_kernel
// (K11's generic kernel, dw_finish).  A workgroup of four waves owns (image, chunk of 32 expanded channels, band of R
// output rows):
//
//   phase 1  the pieces of expand_dw16.h over the s R + 3 - s input rows of the band, a contiguous span of positions of
//            the plane (from the 16-byte boundary at or below its first row), in a loop of its own: the X^T image of
//            a k-tile sits in ONE LDS buffer of a run-time row length (the expands this kernel is for have one or two
//            k-tiles); the next tile's global loads are in flight during the MFMAs.  Wave w runs the 32-position
//            tiles w, w + 4, ...; tiles past the band and all-zero 16-k steps are skipped (EdtBandTiles; the
//            accumulator never holds -0, so they change no bit).
//   between  the chunk's image [32][s R + 3 - s][LW] of the band (a channel's rows padded to 4 elements mod 128, so
//            that the 32 channels of an epilogue store fall into different banks): zeroed first -- the ring columns,
//            and the ring row where the band touches the top (or, at stride 1, the bottom) of the plane -- then filled
//            with the real rows, the neighbour bands' rows included.  Image column j sits at index j + 8.
//   phase 2  per output dw_finish's arithmetic (accumulator from 0.0f, nine fmaf with ky outer and kx inner, acc +
//            bias, activate, settled(), one rounding through K11's element types), no bounds test.  NOT the generic
//            kernel's walk: 8, 16, ... 256 threads per channel (256 / live channels), a thread owns segments of 8 (OW %
//            8 == 0) or 4 horizontally adjacent outputs, its window read from LDS, one 16- or 8-byte store each.
//
// The workgroups of one image run on one XCD, the chunks of a band next to each other, so x is re-read out of that
// XCD's L2.
#include "expand_dw16.h"

namespace mtr {

constexpr int kEdtCM = 32;       // expanded channels per workgroup
constexpr int kEdtColPad = 8;    // image column j of the chunk's image sits at index j + 8
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

// The 32-position tiles of wave `wave` over a band of n_pos staged positions, in k-tile t of Cin = K: tile j is the
// band's tile 4 j + wave; tiles past the band do not run (wave-uniform), nor does a 16-k step past Cin (uniform: it
// would add +0 to an accumulator that is never -0)
struct EdtBandTiles {
  int wave, n_pos, t, K;
  __device__ __forceinline__ int pos(int j) const { return 32 * (4 * j + wave); }
  __device__ __forceinline__ bool step(int s) const { return t * kEdwBK + 16 * s < K; }
  __device__ __forceinline__ bool tile(int j) const { return pos(j) < n_pos; }
};

// FN 32-position tiles per wave, four waves along the positions: BN = 128 FN staged positions per band
template <int DT, int S, int FN>
__global__ __launch_bounds__(256) void expand_dw16_tiles_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w1, const float* __restrict__ bias1,
    const float* __restrict__ wd, const float* __restrict__ bias2, unsigned short* __restrict__ y, EdtGeo g, int B,
    int act1, int act2) {
  using Hh = EdwBits<DT>;
  using T = typename Hh::T;
  constexpr int CM = kEdtCM, BN = 128 * FN, BK = kEdwBK, KS = kEdwKS;
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

  // ---- phase 1: conv1x1_16_kernel's loop over the positions p_base .. p_hi - 1 of one image; this lane's channel:
  // r of the chunk
  const unsigned short* xb = x + (long long)b * K * HW + p_base;
  EdtBandTiles tiles = {wave, n_pos, 0, K};
  EdwXTile<BN> xt;
  edw_f32x16 acc[1][FN];
  edw_clear(acc);
  uint4 wc[1][KS], wnx[1][KS];
  const int n_tiles = (K + BK - 1) / BK;
  xt.load(xb, tid, 0, K, HW, n_pos);
  edw_load_w(wc, w1, m0 + r, M, K, 0, h);
  for (int t = 0; t < n_tiles; ++t) {
    // (the tiles that run; the k columns the image has)
    xt.store(xs, ldk, tid, [&](int p8, int k4) { return 8 * p8 < n_pos32 && 4 * k4 + 8 < ldk; });
    __syncthreads();
    if (t + 1 < n_tiles) {  // in flight during this tile's MFMAs
      xt.load(xb, tid, (t + 1) * BK, K, HW, n_pos);
      edw_load_w(wnx, w1, m0 + r, M, K, (t + 1) * BK, h);
    }
    tiles.t = t;
    edw_mfma_ktile<Hh>(acc, wc, &xs[r * ldk + 8 * h], ldk, tiles);
    __syncthreads();  // the image is read: the next tile's, or the chunk's image, may overwrite it
    if (t + 1 < n_tiles) {
#pragma unroll
      for (int s = 0; s < KS; ++s) wc[0][s] = wnx[0][s];
    }
  }

  // ---- the chunk's image, ring included (LW % 4 == 0, CM % 2 == 0: whole 16-byte groups)
  edw_zero_image(ms, CM * g.plane, tid);
  __syncthreads();
  edw_store_expanded<Hh>(
      acc, act1, bias1, m0, M, r, h, tiles, p_base, p_lo, p_hi,
      [&](int p, int& row, int& col) { row = (int)fastdiv((unsigned)p, g.d_w), col = p - row * g.W; },
      EdwImage{ms, g.plane, g.LW, iy0, kEdtColPad});
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
    if (edw_k11_block_plane(H, W)) return MTR_E_SHAPE;      // (K11's block kernel: other bits)
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
  g.ldk = (Cin <= 16 ? 16 : kEdwBK) + 8;
  g.chunks = (Cmid + kEdtCM - 1) / kEdtCM;
  g.sw8 = g.OW % 8 == 0;
  g.ns = g.OW / (g.sw8 ? 8 : 4);
  g.d_w = make_fastdiv((unsigned)W);
  g.d_ns = make_fastdiv((unsigned)g.ns);
  g.d_chunks = make_fastdiv((unsigned)g.chunks);
  return MTR_OK;
}

template <int DT, int S, int FN>
static int launch_expand_dw16_tiles_cfg(const EdwArgs& a, EdtGeo g, int R) {
  constexpr int BN = 128 * FN;
  g.R = R;
  g.rows_img = S * R + 3 - S;
  g.plane = edt_plane(g, g.rows_img);
  g.bands = (g.OH + R - 1) / R;
  g.d_wgs = make_fastdiv((unsigned)(g.chunks * g.bands));
  auto kern = expand_dw16_tiles_kernel<DT, S, FN>;
  return edw_launch((const void*)kern, a, (size_t)BN * g.ldk * sizeof(unsigned short),
                    (size_t)kEdtCM * g.plane * sizeof(unsigned short), (a.B + 7) / 8 * 8 * g.chunks * g.bands,
                    [&](dim3 grid, size_t lds) {
                      hipLaunchKernelGGL(kern, grid, dim3(256), lds, a.stream, (const unsigned short*)a.x,
                                         (const unsigned short*)a.w1, a.bias1, a.wd, a.bias2, (unsigned short*)a.y, g,
                                         (int)a.B, a.act1, a.act2);
                    });
}

// the only place that maps a shape to the band height and the template parameters: the tallest band up to 8
// (stride 1) or 4 (stride 2) output rows whose input rows fit 512 staged positions; 1024 where that leaves fewer than
// 6 (3) rows -- rows of more than 64 (stride 2: 72) positions
template <int DT, int S>
static int launch_expand_dw16_tiles(const EdwArgs& a, const EdtGeo& g) {
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
static int launch_expand_dw16_tiles_stride(const EdwArgs& a, const EdtGeo& g, int stride) {
  return stride == 1 ? launch_expand_dw16_tiles<DT, 1>(a, g) : launch_expand_dw16_tiles<DT, 2>(a, g);
}

}  // namespace mtr

extern "C" size_t mtr_expand_dw16_tiles_lds_bytes(long long B, int Cin, int Cmid, int H, int W, int stride) {
  mtr::EdtGeo g;
  if (B <= 0 || mtr::expand_dw16_tiles_shape(g, B, Cin, Cmid, H, W, stride) != MTR_OK) return 0;
  // (the tile and LDS rules do not depend on the dtype)
  mtr::EdwArgs a = {};
  a.B = B;
  const int n = mtr::launch_expand_dw16_tiles_stride<MTR_F16>(a, g, stride);
  return n > 0 ? (size_t)n : 0;
}

extern "C" int mtr_expand_dw16_tiles(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                                     const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin,
                                     int Cmid, int H, int W, int stride, void* y, mtr_stream_t stream) {
  const mtr::EdwArgs a = {x, w1, bias1, w_dw, bias_dw, y, nullptr, act1_code, act2_code, B, (hipStream_t)stream};
  mtr::EdtGeo g;
  const int e = mtr::edw_check(a, dtype, Cin, Cmid, -1, [&](int& hw_in, int& hw_out) {
    const int es = mtr::expand_dw16_tiles_shape(g, B, Cin, Cmid, H, W, stride);
    if (es == MTR_OK) hw_in = g.HW, hw_out = g.OH * g.OW;
    return es;
  });
  if (e != MTR_OK) return e;
  if (B == 0) return MTR_OK;
  return dtype == MTR_F16 ? mtr::launch_expand_dw16_tiles_stride<MTR_F16>(a, g, stride)
                          : mtr::launch_expand_dw16_tiles_stride<MTR_BF16>(a, g, stride);
}
