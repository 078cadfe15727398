// K17: the backbone stem -- Preproc (x * 2 - 1) and the dense 3x3, stride-2, padding-1, Cin = 3 convolution
// behind it, with the K10 epilogue folded in -- as one launch, for f32 / f16 / bf16.
//
// Not part of the reference's hot path (like K10 - K16h): the first layer of EfficientNetV2 and MobileNetV3 in the
// backbone's inference copy (backbones.fold_batchnorm(fused_epilogue=True, fuse_stem=True)).  PyTorch-ROCm runs it
// as an elementwise pass, a MIOpen convolution and K10.  Here:
//
//   p[b, ci, iy, ix] = preproc ? rndD(rndX(fma(2, x, -1))) : rndD(x)     inside the image
//                    = 0                                                 outside (the ring is zero AFTER Preproc)
//   y[b, m, oy, ox]  = rndD(act(bias[m] + sum_k w[m, k] * p[b, ci, 2 oy + ky - 1, 2 ox + kx - 1]))
//
// with k = 9 ci + 3 ky + kx, the order of the OIHW weight as it is stored (27 values per output channel: nothing is
// repacked).  rndX rounds to x's dtype, rndD to `dtype` (the tensor the chain would have fed its convolution:
// torch's (x * 2 - 1).to(dtype); x * 2 is exact, so the fma has torch's one rounding).  x is planar [B, 3, H, W] or
// interleaved [B, H, W, 3]; y is [B, Cout, H / 2, W / 2], NCHW-contiguous.
//
// With K = 27 the layer is memory-bound: one read of x, one write of y.  One workgroup (4 waves) computes ALL Cout
// channels of a band of TH output rows of one image, full width:
//   * Input: the band's 2 TH + 1 input rows of the three channels are staged once into LDS as planar [ci][row][column]
//     rows of `dtype` elements, Preproc applied and the input cast on the way in.  A loader unit is 8 pixels (W % 8 ==
//     0): one channel's 8 elements of a planar row, or the 24 interleaved elements, de-interleaved in registers.  Image
//     column ix sits at LDS column ix + 8; the 8-column group in front of each row and the row above the image are
//     zero-filled, so the k loop has no bounds tests.  Full-width bands have no horizontal halo; vertically one input
//     row in 2 TH + 1 is read by two workgroups.
//   * The whole weight is in registers: lane (r, h) = (lane & 31, lane >> 5) holds, for each tile of 32 output
//     channels, row r's k group of every MFMA step.
//   * 16-bit: v_mfma_f32_32x32x16_{f16,bf16}, two steps, K padded from 27 to 32 with zeros on BOTH operands.  The A
//     fragment (32 consecutive output positions of the band x 8 k) is gathered from LDS with 2-byte reads at
//     the lane's position + a per-k offset (consecutive positions are 4 bytes apart: no bank conflicts).
//     f32: v_mfma_f32_32x32x2_f32, 14 steps (K padded to 28): the k-ordered fmaf chain of the guide, exact f32
//     products, the same accumulator layout, hence the same epilogue.  About half the f32 byte floor's time; VALU
//     FMAs would cost the same rate and every address twice.
//   * A wave takes 32 FN consecutive positions (FN = 2 for 16 bits, 1 for f32) per pass.  Output positions of a
//     full-width band are CONTIGUOUS in each channel plane of y: the rounded tile is turned through the wave's own
//     LDS rows and each store instruction writes 128-byte runs of 4 (f32: 8) channel rows.
//
// k runs in one order -- the MFMA steps 0, 1, ... over k = 0 .. 26 -- whatever the band, the batch index or the
// layout; no atomics, no workspace: the same inputs give the same bits.
#include "common.h"

namespace mtr {

typedef float st_f32x16 __attribute__((ext_vector_type(16)));

template <int T> struct StemT;
template <> struct StemT<MTR_F32> {
  typedef float E;
  static __device__ __forceinline__ float f32(E v) { return v; }
  static __device__ __forceinline__ E rnd(float f) { return f; }
};
template <> struct StemT<MTR_F16> {
  typedef _Float16 E;
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ float f32(E v) { return (float)v; }
  static __device__ __forceinline__ E rnd(float f) { return (_Float16)f; }
  static __device__ __forceinline__ st_f32x16 mfma(v8 a, v8 b, st_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};
template <> struct StemT<MTR_BF16> {
  typedef __bf16 E;
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ float f32(E v) { return (float)v; }
  static __device__ __forceinline__ E rnd(float f) { return (__bf16)f; }
  static __device__ __forceinline__ st_f32x16 mfma(v8 a, v8 b, st_f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};

// the geometry of one launch, computed on the host (stem_geometry) and used by both sides
struct StemGeo {
  int M, H, W, Ho, Wo;
  int TH;      // output rows per band (the last band of a map may have fewer)
  int R0, LW;  // staged rows per channel (2 TH + 1) and their length in elements (W + 8)
  FastDiv d_gw1, d_r0, d_wo;  // by W / 8 + 1, R0, Wo
};

constexpr int kStemThreads = 256;
constexpr int kStemK = 27;

// N elements moved as one access (8 or 16 bytes; 32 bytes as two): no padding behind the elements
template <typename E, int N> struct alignas(sizeof(E) * N < 16 ? sizeof(E) * N : 16) StemPack { E e[N]; };
static_assert(sizeof(StemPack<_Float16, 4>) == 8 && sizeof(StemPack<float, 4>) == 16 && sizeof(StemPack<float, 8>) == 32,
              "a pack is exactly its elements");

// 32 FM output channels; XT: x's dtype, DT: the dtype of the weight and of y; IL: x is interleaved [H][W][3]
template <int XT, int DT, int IL, int FM>
__global__ __launch_bounds__(kStemThreads) void stem_conv_kernel(
    const void* __restrict__ x_, const void* __restrict__ w_, const float* __restrict__ bias, void* __restrict__ y_,
    StemGeo g, int act, int preproc) {
  using X = StemT<XT>;
  using D = StemT<DT>;
  typedef typename X::E XE;
  typedef typename D::E DE;
  constexpr bool F32 = DT == MTR_F32;
  constexpr int FN = F32 ? 1 : 2;
  constexpr int NT = kStemThreads;
  constexpr int TP = 32 * FN;       // positions per wave and pass
  constexpr int LDP = 32 * FN + 4;  // elements per channel row of the epilogue's turn
  extern __shared__ __attribute__((aligned(16))) unsigned char stem_smem[];
  DE* xs = reinterpret_cast<DE*>(stem_smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int M = g.M, H = g.H, W = g.W, Wo = g.Wo, R0 = g.R0, LW = g.LW;
  const int plane_l = R0 * LW;  // LDS elements per channel
  DE* ys = xs + 3 * plane_l + wave * (32 * LDP);
  const int oy0 = blockIdx.x * g.TH;
  const int th = min(g.TH, g.Ho - oy0);
  const long long b = blockIdx.y;

  // ---- stage the band: [3][R0 rows][LW columns], input rows 2 oy0 - 1 ..., image column ix at LDS column ix + 8
  {
    constexpr int NCH = IL ? 3 : 1;                     // channels per loader unit
    constexpr int XN = 16 / (int)sizeof(XE);            // x elements per 16-byte load
    constexpr int XV = NCH * 8 / XN;                    // 16-byte loads per unit
    constexpr int U = IL ? 2 : 4;                       // units in flight per thread
    typedef StemPack<XE, XN> XP;
    const XE* xb = reinterpret_cast<const XE*>(x_) + b * 3LL * H * W;
    const int GW1 = (W >> 3) + 1, iy0 = 2 * oy0 - 1;
    const int n_units = (IL ? 1 : 3) * R0 * GW1;
    for (int u0 = 0; u0 < n_units; u0 += U * NT) {
      XP raw[U][XV];
      int dst[U];
      bool inside[U];
#pragma unroll
      for (int k = 0; k < U; ++k) {
        const int u = u0 + k * NT + tid;
        dst[k] = -1;
        inside[k] = false;
#pragma unroll
        for (int v = 0; v < XV; ++v)
#pragma unroll
          for (int e = 0; e < XN; ++e) raw[k][v].e[e] = XE(0.0f);
        if (u < n_units) {
          // unit -> (channel c, band row ly, column group gx): the groups of a row are neighbours in the wave
          const int rest = (int)fastdiv((unsigned)u, g.d_gw1), gx = u - rest * GW1 - 1;
          const int c = (int)fastdiv((unsigned)rest, g.d_r0), ly = rest - c * R0;  // (interleaved: c == 0)
          dst[k] = (c * R0 + ly) * LW + 8 + 8 * gx;
          const int iy = iy0 + ly;
          if (gx >= 0 && iy >= 0 && iy < H) {  // (W % 8 == 0: the whole group is inside)
            inside[k] = true;
            const XE* p = IL ? xb + ((long long)iy * W + 8 * gx) * 3 : xb + ((long long)c * H + iy) * W + 8 * gx;
#pragma unroll
            for (int v = 0; v < XV; ++v) raw[k][v] = reinterpret_cast<const XP*>(p)[v];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k) {
        if (dst[k] < 0) continue;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          StemPack<DE, 8> o;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const int idx = IL ? 3 * e + c : e;
            XE xe = raw[k][idx / XN].e[idx % XN];
            // torch's x * 2 - 1 in x's dtype: x * 2 is exact, so one fma has its single rounding
            if (preproc) xe = X::rnd(__builtin_fmaf(2.0f, X::f32(xe), -1.0f));
            o.e[e] = inside[k] ? D::rnd(X::f32(xe)) : DE(0.0f);  // the ring is zero AFTER Preproc
          }
          *reinterpret_cast<StemPack<DE, 8>*>(xs + dst[k] + c * plane_l) = o;
        }
      }
    }
  }

  // ---- the weight, in registers: row m = 32 i + r, this lane's k of every step (zero past k = 26 and past Cout)
  const DE* w = reinterpret_cast<const DE*>(w_);
  constexpr int NS = F32 ? 14 : 2;   // MFMA steps
  constexpr int KL = F32 ? 1 : 8;    // k per lane and step
  DE wr[FM][NS][KL];
  int koff[NS][KL];  // the LDS offset of tap k from the lane's position (0 for the padded k)
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int j = 0; j < KL; ++j) {
      const int k = F32 ? 2 * s + h : 16 * s + 8 * h + j;
      const int ci = k / 9, rem = k - 9 * ci, ky = rem / 3, kx = rem - 3 * ky;
      koff[s][j] = k < kStemK ? (ci * R0 + ky) * LW + kx : 0;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int m = 32 * i + r;
        wr[i][s][j] = (m < M && k < kStemK) ? w[m * kStemK + k] : DE(0.0f);
      }
    }
  __syncthreads();

  const int npos = th * Wo, ntiles = (npos + TP - 1) / TP;
  DE* y = reinterpret_cast<DE*>(y_) + ((b * M) * g.Ho + oy0) * (long long)Wo;
  const long long chan = (long long)g.Ho * Wo;
  // (the trip count is the same in every wave -- the epilogue's barriers; a wave past the last tile computes the
  // band's last position again and stores nothing)
  for (int t0 = 0; t0 < ntiles; t0 += NT / 64) {
    const int q0 = (t0 + wave) * TP;
    st_f32x16 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int q = min(q0 + 32 * j + r, npos - 1);
      const int oyl = (int)fastdiv((unsigned)q, g.d_wo), ox = q - oyl * Wo;
      const DE* pa = xs + (2 * oyl) * LW + 2 * ox + 7;  // tap (0, 0) of this lane's position
      if constexpr (F32) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          float a = pa[koff[s][0]];
          if (2 * s + 1 >= kStemK && h) a = 0.0f;
#pragma unroll
          for (int i = 0; i < FM; ++i)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wr[i][s][0], acc[i][j], 0, 0, 0);
        }
      } else {
        typedef typename D::v8 v8;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          v8 a;
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            DE v = pa[koff[s][jj]];
            if (16 * s + 8 + jj >= kStemK && h) v = DE(0.0f);  // the padded k: zero on both operands
            a[jj] = v;
          }
#pragma unroll
          for (int i = 0; i < FM; ++i) {
            v8 wv;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) wv[jj] = wr[i][s][jj];
            acc[i][j] = D::mfma(a, wv, acc[i][j]);
          }
        }
      }
    }

    // ---- epilogue: lane holds channel 32 i + r, positions q0 + 32 j + 8 qq + 4 h + 0..3.  Bias and activation in
    // registers, one rounding; the tile then goes through this wave's LDS rows ([channel][position]) so that the
    // global stores run along the channel rows, which are contiguous in y over the whole band.
    auto epilogue = [&](auto tag) {
      constexpr int ACT = decltype(tag)::value;
      constexpr int PL = 8 * FN, CH = 64 / PL;  // lanes per channel row, channel rows per store instruction
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int mb = 32 * i, m = mb + r;
        const float bm = m < M ? bias[m] : 0.0f;
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            StemPack<DE, 4> o;
            // (settled: the activation's last product is rounded to f32 before the output rounding, as K10's is)
#pragma unroll
            for (int e = 0; e < 4; ++e) o.e[e] = D::rnd(settled(activate<ACT>(acc[i][j][4 * qq + e] + bm)));
            *reinterpret_cast<StemPack<DE, 4>*>(ys + r * LDP + 32 * j + 8 * qq + 4 * h) = o;
          }
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 32 / CH; ++pass) {
          const int c = pass * CH + lane / PL, pp = (lane % PL) * 4;
          const StemPack<DE, 4> o = *reinterpret_cast<const StemPack<DE, 4>*>(ys + c * LDP + pp);
          if (mb + c < M && q0 + pp < npos)  // (npos % 4 == 0: the whole group is inside)
            *reinterpret_cast<StemPack<DE, 4>*>(y + (mb + c) * chan + q0 + pp) = o;
        }
        __syncthreads();  // the rows are rewritten by the next channel tile / pass
      }
    };
    // wave-uniform.  Written out: behind the shared with_act() the f32 instantiations come out one instruction
    // shorter, which is not the same code
    switch (act) {
      case kActRelu: epilogue(ActTag<kActRelu>()); break;
      case kActSilu: epilogue(ActTag<kActSilu>()); break;
      case kActHardswish: epilogue(ActTag<kActHardswish>()); break;
      default: epilogue(ActTag<kActNone>()); break;
    }
  }
}

constexpr size_t kStemMaxLds = 160 * 1024;

// The band: TH = the largest power of two <= min(32, 1024 / Wo) output rows (at least 1), full width.
inline int stem_band_rows(int Wo) {
  const int cap = std::min(32, std::max(1, 1024 / Wo));
  int th = 1;
  while (2 * th <= cap) th *= 2;
  return th;
}

// the shape rules of the entry (MTR_E_SHAPE: the caller keeps the chain); fills g
static int stem_shape(StemGeo& g, long long B, int Cin, int Cout, int H, int W) {
  if (B < 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (Cin != 3 || H % 2 || W % 8 || Cout % 8 || Cout > 64) return MTR_E_SHAPE;
  if (B > 65535 || 3LL * H * W > 0x7fffffffLL || (long long)Cout * (H / 2) * (W / 2) > 0x7fffffffLL)
    return MTR_E_SHAPE;
  g = StemGeo{};
  g.M = Cout, g.H = H, g.W = W, g.Ho = H / 2, g.Wo = W / 2;
  g.TH = stem_band_rows(g.Wo);
  g.R0 = 2 * g.TH + 1, g.LW = W + 8;
  g.d_gw1 = make_fastdiv((unsigned)(W / 8 + 1));
  g.d_r0 = make_fastdiv((unsigned)g.R0);
  g.d_wo = make_fastdiv((unsigned)g.Wo);
  return MTR_OK;
}

// LDS bytes of one workgroup: the staged band and the four waves' epilogue rows; 0 where it does not fit
static size_t stem_lds_bytes(const StemGeo& g, int dtype) {
  const size_t es = dtype == MTR_F32 ? 4 : 2;
  const size_t ldp = dtype == MTR_F32 ? 36 : 68;
  const size_t n = (3 * (size_t)g.R0 * g.LW + (kStemThreads / 64) * 32 * ldp) * es;
  return n <= kStemMaxLds ? n : 0;
}

template <int XT, int DT, int IL, int FM>
static int launch_stem_cfg(const void* x, const void* w, const float* bias, void* y, int act, int preproc,
                           long long B, const StemGeo& g, hipStream_t stream) {
  const size_t lds = stem_lds_bytes(g, DT);
  auto kern = stem_conv_kernel<XT, DT, IL, FM>;
  if (lds > 64 * 1024) {
    const int e = allow_dynamic_lds((const void*)kern, kStemMaxLds);
    if (e != MTR_OK) return e;
  }
  const dim3 grid((unsigned)((g.Ho + g.TH - 1) / g.TH), (unsigned)B), block(kStemThreads);
  MTR_CLEAR_STALE();
  hipLaunchKernelGGL(kern, grid, block, lds, stream, x, w, bias, y, g, act, preproc);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

template <int XT, int DT>
static int launch_stem(const void* x, int layout, const void* w, const float* bias, void* y, int act, int preproc,
                       long long B, const StemGeo& g, hipStream_t s) {
  if (layout == MTR_NHWC) {
    if (g.M <= 32) return launch_stem_cfg<XT, DT, 1, 1>(x, w, bias, y, act, preproc, B, g, s);
    return launch_stem_cfg<XT, DT, 1, 2>(x, w, bias, y, act, preproc, B, g, s);
  }
  if (g.M <= 32) return launch_stem_cfg<XT, DT, 0, 1>(x, w, bias, y, act, preproc, B, g, s);
  return launch_stem_cfg<XT, DT, 0, 2>(x, w, bias, y, act, preproc, B, g, s);
}

static bool stem_dtypes_ok(int x_dtype, int dtype) {
  if (dtype != MTR_F32 && dtype != MTR_F16 && dtype != MTR_BF16) return false;
  return x_dtype == dtype || (x_dtype == MTR_F32 && dtype != MTR_F32);
}

}  // namespace mtr

extern "C" size_t mtr_stem_conv_lds_bytes(int dtype, long long B, int Cin, int Cout, int H, int W) {
  mtr::StemGeo g;
  if (dtype != MTR_F32 && dtype != MTR_F16 && dtype != MTR_BF16) return 0;
  if (mtr::stem_shape(g, B, Cin, Cout, H, W) != MTR_OK) return 0;
  return mtr::stem_lds_bytes(g, dtype);
}

extern "C" int mtr_stem_conv3x3s2(const void* x, int x_dtype, int layout, const void* weight, const float* bias,
                                  int dtype, int act, int preproc, long long B, int Cin, int Cout, int H, int W,
                                  void* y, mtr_stream_t stream) {
  using namespace mtr;
  if (!x || !weight || !bias || !y) return MTR_E_NULL;
  if (!stem_dtypes_ok(x_dtype, dtype)) return MTR_E_DTYPE;
  StemGeo g;
  const int e = stem_shape(g, B, Cin, Cout, H, W);
  if (e != MTR_OK) return e;
  if (stem_lds_bytes(g, dtype) == 0) return MTR_E_SHAPE;
  if (act < kActNone || act > kActHardswish || (layout != MTR_NCHW && layout != MTR_NHWC) ||
      (preproc != 0 && preproc != 1))
    return MTR_E_PARAM;
  const size_t xs = x_dtype == MTR_F32 ? 4 : 2, ds = dtype == MTR_F32 ? 4 : 2;
  if (((uintptr_t)x % 16) || ((uintptr_t)y % 16) || ((uintptr_t)weight % ds) || ((uintptr_t)bias % 4))
    return MTR_E_ALIGN;
  // y is written while x is still read by other workgroups: the two must not overlap
  const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)B * 3 * H * W * xs;
  const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (size_t)B * Cout * (H / 2) * (W / 2) * ds;
  if (x == y || (x0 < y1 && y0 < x1)) return MTR_E_PARAM;
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) return MTR_OK;  // nothing to do
  if (dtype == MTR_F32) return launch_stem<MTR_F32, MTR_F32>(x, layout, weight, bias, y, act, preproc, B, g, s);
  if (dtype == MTR_F16) {
    if (x_dtype == MTR_F32) return launch_stem<MTR_F32, MTR_F16>(x, layout, weight, bias, y, act, preproc, B, g, s);
    return launch_stem<MTR_F16, MTR_F16>(x, layout, weight, bias, y, act, preproc, B, g, s);
  }
  if (x_dtype == MTR_F32) return launch_stem<MTR_F32, MTR_BF16>(x, layout, weight, bias, y, act, preproc, B, g, s);
  return launch_stem<MTR_BF16, MTR_BF16>(x, layout, weight, bias, y, act, preproc, B, g, s);
}
