// K28h: the function of expand_dw16.h for the depthwise 5x5 layers (stride 1 or 2, zero padding 2 all round), with
// the mean: the 1x1 expand of an MBConv block (K13h, conv1x1_16.hip) and the depthwise 5x5 layer behind it (K15,
// depthwise5x5.hip) as ONE launch, the expanded activation kept in LDS.  y and the mean have the bits of that chain.
//
// Not part of the reference's hot path (like K10 - K27h): backbones.fold_batchnorm(dtype=f16 / bf16,
// fuse_expand_depthwise5x5=True).  A workgroup of four waves owns CM = 32 WM expanded channels of one image over the
// WHOLE plane (the mean needs it: no bands):
//
//   first    the slice's image [c][PH][LW] of 16-bit values is zeroed: row i of the plane is image row i + 2, column j
//            sits at index j + 4 (8-byte aligned stores of four positions), so the ring of zeros is two rows and at
//            least two columns wide on every side.  PH and LW follow K15's PH / PW rule: the last unit's window stays
//            inside the image, and phase 2 needs no bounds test.  Widening 16 bits to f32 is exact, so K15's f32 tile
//            and this image hold the same values.
//   phase 1  edw_gemm_span in passes of 256 positions (8 position tiles: WN waves x FN tiles), so a 32x32 plane never
//            holds more than FN accumulator tiles per wave; each pass's K13h epilogue (edw_store_expanded) goes into
//            the image.  The tiles past the plane run no MFMA and store nothing.  The X^T staging buffers lie BESIDE
//            the image.
//   phase 2  depthwise5x5_kernel's units and arithmetic: a lane computes a unit of RB x 4 outputs (RB 4 at stride 1, 2
//            at stride 2) from 8-byte LDS reads of its window rows; per output the accumulator starts at 0.0f, 25 fmaf
//            with ky outer and kx inner, activate(acc + bias) -- no settled(): K15 has none --, one rounding.  The
//            mean in K15's order: per unit the rows in order, each row summed from 0.0f over its four rounded outputs
//            and added where oy < OH; partial[unit] in LDS; lane l of G adds partial[l], partial[l + G], ... from
//            0.0f; the xor butterfly G / 2 .. 1; times 1.0f / (OH OW).  The depthwise weights and the unit sums take
//            the place of the staging buffers, which are dead by then.
//
// No atomics, no split-K, no workspace.  The workgroup-to-image mapping is edw_image_chunk's, as K25h's.
#include "expand_dw16.h"

namespace mtr {

constexpr int kEdkBN = 256;          // positions per pass of phase 1
constexpr int kEdkColPad = 4;        // column j of the plane at index j + 4 of an image row
constexpr int kEdkRowPad = 2;        // row i of the plane is image row i + 2
constexpr int kEdkWeightSlot = 28;   // 25 taps + the bias, padded to whole float4 (K15's slot)
constexpr size_t kEdkStageBytes = (size_t)2 * kEdkBN * kEdwLDK * sizeof(unsigned short);

struct EdkGeo {
  int Cin, Cmid, H, W, HW, stride, OH, OW;
  int LW, PH, plane;    // elements per row, rows and elements per channel of the slice's image
  int chunks;           // workgroups per image = ceil(Cmid / CM)
  int xcd_map;          // 1: the chunks of one image on one XCD
  int UW, units;        // units (RB x 4 output blocks) per row of units / per plane
  int G;                // lanes that reduce one plane's sum (K15's: a power of two <= 64)
  int n_pass;           // passes of phase 1 = ceil(HW / 256)
  float inv_hw;
  FastDiv d_w, d_units, d_uw;
};

// The 32-position tiles of a wave in one pass: FN in a row from `first`; those at or past n_pos (the end of the plane)
// run no MFMA -- their accumulators stay zero and edw_store_expanded stores nothing of them.
struct EdkPassTiles {
  int first, n_pos;
  __device__ __forceinline__ int pos(int j) const { return first + 32 * j; }
  __device__ __forceinline__ bool step(int) const { return true; }
  __device__ __forceinline__ bool tile(int j) const { return first + 32 * j < n_pos; }
};

template <int DT, int WM, int STRIDE>
__global__ __launch_bounds__(256) void expand_dw16_k5_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ w1, const float* __restrict__ bias1,
    const float* __restrict__ wd, const float* __restrict__ bias2, unsigned short* __restrict__ y,
    float* __restrict__ row_mean, EdkGeo g, int B, int act1, int act2) {
  using Hh = EdwBits<DT>;
  using T = typename Hh::T;
  constexpr int WN = 4 / WM, FN = kEdkBN / (32 * WN), CM = 32 * WM;
  constexpr int RB = STRIDE == 1 ? 4 : 2;        // output rows of a unit
  constexpr int NR = (RB - 1) * STRIDE + 5;       // rows of its window
  constexpr int NC = STRIDE == 1 ? 3 : 4;         // 8-byte groups of a window row: indices s ox0 .. s ox0 + 4 NC - 1
  extern __shared__ __attribute__((aligned(16))) unsigned short edk_lds[];
  unsigned short* ms = edk_lds;                    // [CM][PH][LW], the slice of the expanded activation
  unsigned short* xs = edk_lds + CM * g.plane;     // phase 1: [2][256 * LDK], the X^T image of a k-tile
  float* wts = reinterpret_cast<float*>(xs);       // phase 2: [CM][28] depthwise weights and bias
  float* partial = wts + CM * kEdkWeightSlot;      //          [CM][units] unit sums

  int b, chunk;
  edw_image_chunk(g.xcd_map, g.chunks, b, chunk);
  if (b >= B) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int r = lane & 31, h = lane >> 5;
  const int M = g.Cmid, K = g.Cin, HW = g.HW;
  const int m0 = chunk * CM;

  // ---- the image, zeroed: ring and dead channels included (CM % 32 == 0, LW % 4 == 0: whole 16-byte groups)
  edw_zero_image(ms, CM * g.plane, tid);
  __syncthreads();

  // ---- phase 1 in passes; this lane's channel: cl of the slice
  const int cl = wm * 32 + r;
  const unsigned short* xb = x + (long long)b * K * HW;
  for (int pass = 0; pass < g.n_pass; ++pass) {
    const int p0 = pass * kEdkBN;
    const EdkPassTiles tiles = {wn * (32 * FN), HW - p0};
    edw_f32x16 acc[1][FN];
    edw_gemm_span<Hh, kEdkBN>(acc, xs, xb + p0, w1, m0 + cl, M, K, HW, HW - p0, tid, tiles);
    edw_store_expanded<Hh>(
        acc, act1, bias1, m0, M, cl, h, tiles, p0, 0, HW,
        [&](int p, int& row, int& col) { row = (int)fastdiv((unsigned)p, g.d_w), col = p - row * g.W; },
        EdwImage{ms, g.plane, g.LW, -kEdkRowPad, kEdkColPad});
  }
  // (the last pass ended its GEMM on a barrier: the staging buffers are free)
  const int live = M - m0 < CM ? M - m0 : CM;  // the slice's channels below Cmid: phase 2 touches no other
  for (int i = tid; i < live * 26; i += 256) {
    const int q = i / 26, k = i - q * 26;
    wts[q * kEdkWeightSlot + k] = k < 25 ? wd[(m0 + q) * 25 + k] : bias2[m0 + q];
  }
  __syncthreads();

  // ---- phase 2: depthwise5x5_kernel's units and arithmetic, the window from LDS (the ring is zero: no masks)
  const int live_units = live * g.units;
  auto depthwise = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
    struct alignas(4 * sizeof(T)) V4 { T v[4]; };
    for (int u = tid; u < live_units; u += 256) {
      const int q = (int)fastdiv((unsigned)u, g.d_units);
      const int v = u - q * g.units;
      const int uy = (int)fastdiv((unsigned)v, g.d_uw);
      const int oy0 = uy * RB, ox0 = (v - uy * g.UW) << 2;
      float wk[kEdkWeightSlot];
#pragma unroll
      for (int k = 0; k < kEdkWeightSlot / 4; ++k) {
        const float4 t = reinterpret_cast<const float4*>(wts + q * kEdkWeightSlot)[k];
        wk[4 * k] = t.x; wk[4 * k + 1] = t.y; wk[4 * k + 2] = t.z; wk[4 * k + 3] = t.w;
      }
      // rows s oy0 - 2 .. of the plane = rows s oy0 .. of the image; columns s ox0 - 2 .. = indices s ox0 + 2 ..
      const unsigned short* win = ms + q * g.plane + oy0 * STRIDE * g.LW + ox0 * STRIDE;
      float acc[RB][4];
#pragma unroll
      for (int a = 0; a < RB; ++a)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[a][o] = 0.0f;
#pragma unroll
      for (int rr = 0; rr < NR; ++rr) {
        float in[NC * 4];
#pragma unroll
        for (int n = 0; n < NC; ++n) {
          const V4 t = reinterpret_cast<const V4*>(win + rr * g.LW)[n];
#pragma unroll
          for (int e = 0; e < 4; ++e) in[4 * n + e] = to_f32(t.v[e]);
        }
#pragma unroll
        for (int a = 0; a < RB; ++a) {
          const int ky = rr - a * STRIDE;  // (compile-time after unrolling)
          if (ky < 0 || ky > 4) continue;
#pragma unroll
          for (int kx = 0; kx < 5; ++kx)
#pragma unroll
            for (int o = 0; o < 4; ++o)
              acc[a][o] = fmaf(in[o * STRIDE + kx + kEdkColPad - 2], wk[ky * 5 + kx], acc[a][o]);
        }
      }
      unsigned short* yp = y + ((size_t)b * (size_t)M + (size_t)(m0 + q)) * (size_t)(g.OH * g.OW) + ox0;
      float sum = 0.0f;
#pragma unroll
      for (int a = 0; a < RB; ++a) {
        V4 out;
        const bool row_ok = oy0 + a < g.OH;
        float s = 0.0f;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          // ONE 16-bit value, stored and summed: K15's f16 kernels round the activation's last product (silu,
          // hardswish) and the conversion as one operation (v_fma_mixlo_f16); left to itself the compiler gave this
          // kernel a second, twice-rounded copy for the store (common.h's settled() tells the same story for K11)
          unsigned bits = __builtin_bit_cast(unsigned short, T(activate<ACT>(acc[a][o] + wk[25])));
          asm("" : "+v"(bits));
          out.v[o] = __builtin_bit_cast(T, (unsigned short)bits);
          s += to_f32(out.v[o]);
        }
        if (row_ok) {
          sum += s;
          *reinterpret_cast<V4*>(yp + (oy0 + a) * g.OW) = out;
        }
      }
      partial[u] = sum;
    }
  };
  with_act(act2, depthwise);
  if (!row_mean) return;  // (uniform over the grid)
  __syncthreads();
  const int l = tid & (g.G - 1), per_pass = 256 / g.G;
  for (int base = 0; base < CM; base += per_pass) {  // (uniform over the workgroup)
    const int q = base + tid / g.G;
    const bool on = q < live;
    float s = 0.0f;
    if (on)
      for (int i = l; i < g.units; i += g.G) s += partial[q * g.units + i];
    for (int m = g.G >> 1; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (on && l == 0) row_mean[(size_t)b * (size_t)M + (size_t)(m0 + q)] = s * g.inv_hw;
  }
}

// the shape rules of the entry (MTR_E_SHAPE: the caller keeps the two-kernel chain); fills g
static int expand_dw16_k5_shape(EdkGeo& g, long long B, int Cin, int Cmid, int H, int W, int stride) {
  if (B < 0 || Cin <= 0 || Cmid <= 0 || H <= 0 || W <= 0) return MTR_E_SHAPE;
  if (stride != 1 && stride != 2) return MTR_E_SHAPE;
  // 16-byte groups of k and of positions; four positions of the expand's epilogue inside one row of the plane
  if (Cin % 8 || (H * (long long)W) % 8 || W % 4) return MTR_E_SHAPE;
  if (H + 4 > 112 || W + 4 > 112) return MTR_E_SHAPE;  // K15's bound on the padded plane
  const int OH = (H + 4 - 5) / stride + 1, OW = (W + 4 - 5) / stride + 1;  // as mtr_depthwise5x5_bias_act_padded
  if (OW % 4 != 0) return MTR_E_SHAPE;
  if (B * Cmid >= (1LL << 30)) return MTR_E_SHAPE;  // (K15's own limit)
  const int RB = stride == 1 ? 4 : 2, NC = stride == 1 ? 3 : 4;
  g = EdkGeo{};
  g.Cin = Cin, g.Cmid = Cmid, g.H = H, g.W = W, g.HW = H * W, g.stride = stride, g.OH = OH, g.OW = OW;
  const int UH = (OH + RB - 1) / RB;
  g.UW = OW / 4;
  g.units = UH * g.UW;
  // K15's PH / PW rule: what the windows read (here in whole 8-byte groups from index stride ox0), or the padded plane
  const int rows = (UH * RB - 1) * stride + 5, cols = stride * (OW - 4) + 4 * NC;
  g.PH = rows > H + 4 ? rows : H + 4;
  g.LW = ((cols > W + kEdkColPad + 2 ? cols : W + kEdkColPad + 2) + 3) & ~3;
  g.plane = g.PH * g.LW;
  g.xcd_map = 1;
  g.G = 1;
  while (g.G < 64 && g.G < g.units) g.G <<= 1;
  g.n_pass = (g.HW + kEdkBN - 1) / kEdkBN;
  g.inv_hw = 1.0f / (float)(OH * OW);
  g.d_w = make_fastdiv((unsigned)W);
  g.d_units = make_fastdiv((unsigned)g.units);
  g.d_uw = make_fastdiv((unsigned)g.UW);
  return MTR_OK;
}

// the LDS of a workgroup of CM channels: the image, and beside it the staging buffers of phase 1 or, in their place, the
// weights and unit sums of phase 2
static size_t expand_dw16_k5_lds(const EdkGeo& g, int CM) {
  const size_t tail = (size_t)CM * (kEdkWeightSlot + g.units) * sizeof(float);
  return (size_t)CM * g.plane * sizeof(unsigned short) + (tail > kEdkStageBytes ? tail : kEdkStageBytes);
}

template <int DT, int WM, int STRIDE>
static int launch_expand_dw16_k5_cfg(const EdwArgs& a, EdkGeo g) {
  constexpr int CM = 32 * WM;
  g.chunks = (g.Cmid + CM - 1) / CM;
  auto kern = expand_dw16_k5_kernel<DT, WM, STRIDE>;
  // (edw_launch takes the larger of its two sizes: here the image and what lies beside it are one sum)
  return edw_launch((const void*)kern, a, expand_dw16_k5_lds(g, CM), 0,
                    (g.xcd_map ? (a.B + 7) / 8 * 8 : a.B) * g.chunks, [&](dim3 grid, size_t lds) {
                      hipLaunchKernelGGL(kern, grid, dim3(256), lds, a.stream, (const unsigned short*)a.x,
                                         (const unsigned short*)a.w1, a.bias1, a.wd, a.bias2, (unsigned short*)a.y,
                                         a.row_mean, g, (int)a.B, a.act1, a.act2);
                    });
}

// The only place that chooses CM for a plane: 64 channels where Cmid has more than 32 and the LDS leaves room for a
// second workgroup on the CU (80 KiB; the compiler reports both configurations under 256 registers); else 32 channels in
// up to 160 KiB (the 32x32 planes); past that MTR_E_SHAPE.  The 80 KiB line is a supposition -- one workgroup's phase 2,
// which waits on LDS, beside another's phase 1 -- and no other line has been timed.  (128 channels -- eight accumulator
// tiles a wave -- compiled to 372 registers and was dropped on that figure, untimed.)
static int expand_dw16_k5_wm(const EdkGeo& g) {
  return g.Cmid > 32 && expand_dw16_k5_lds(g, 64) <= kEdwMaxLds / 2 ? 2 : 1;
}

template <int DT, int STRIDE>
static int launch_expand_dw16_k5_s(const EdwArgs& a, const EdkGeo& g) {
  return expand_dw16_k5_wm(g) == 2 ? launch_expand_dw16_k5_cfg<DT, 2, STRIDE>(a, g)
                                   : launch_expand_dw16_k5_cfg<DT, 1, STRIDE>(a, g);
}

template <int DT>
static int launch_expand_dw16_k5(const EdwArgs& a, const EdkGeo& g) {
  return g.stride == 1 ? launch_expand_dw16_k5_s<DT, 1>(a, g) : launch_expand_dw16_k5_s<DT, 2>(a, g);
}

}  // namespace mtr

extern "C" size_t mtr_expand_dw16_k5_lds_bytes(long long B, int Cin, int Cmid, int H, int W, int stride) {
  mtr::EdkGeo g;
  if (B <= 0 || mtr::expand_dw16_k5_shape(g, B, Cin, Cmid, H, W, stride) != MTR_OK) return 0;
  // (the slice and LDS rules do not depend on the dtype)
  mtr::EdwArgs a = {};
  a.B = B;
  const int n = mtr::launch_expand_dw16_k5<MTR_F16>(a, g);
  return n > 0 ? (size_t)n : 0;
}

extern "C" int mtr_expand_dw16_k5_opts(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                                       const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin,
                                       int Cmid, int H, int W, int stride, void* y, float* row_mean,
                                       mtr_stream_t stream, int mapping) {
  const mtr::EdwArgs a = {x, w1, bias1, w_dw, bias_dw, y, row_mean, act1_code, act2_code, B, (hipStream_t)stream};
  mtr::EdkGeo g;
  const int e = mtr::edw_check(a, dtype, Cin, Cmid, mapping, [&](int& hw_in, int& hw_out) {
    const int es = mtr::expand_dw16_k5_shape(g, B, Cin, Cmid, H, W, stride);
    if (es != MTR_OK) return es;
    hw_in = g.HW, hw_out = g.OH * g.OW;
    // the LDS rule is a shape rule too: refused here, before the parameters and the alignment, as the query says it
    return mtr::expand_dw16_k5_lds(g, 32 * mtr::expand_dw16_k5_wm(g)) > mtr::kEdwMaxLds ? (int)MTR_E_SHAPE : (int)MTR_OK;
  });
  if (e != MTR_OK) return e;
  if (B == 0) return MTR_OK;
  if (mapping >= 0) g.xcd_map = mapping;
  return dtype == MTR_F16 ? mtr::launch_expand_dw16_k5<MTR_F16>(a, g) : mtr::launch_expand_dw16_k5<MTR_BF16>(a, g);
}

extern "C" int mtr_expand_dw16_k5(const void* x, int dtype, const void* w1, const float* bias1, int act1_code,
                                  const float* w_dw, const float* bias_dw, int act2_code, long long B, int Cin, int Cmid,
                                  int H, int W, int stride, void* y, float* row_mean, mtr_stream_t stream) {
  return mtr_expand_dw16_k5_opts(x, dtype, w1, bias1, act1_code, w_dw, bias_dw, act2_code, B, Cin, Cmid, H, W, stride,
                                 y, row_mean, stream, -1);
}
