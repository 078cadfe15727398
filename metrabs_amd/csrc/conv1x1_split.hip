// K20: a 1x1 stride-1 NCHW convolution of f32 tensors on the bf16 matrix cores, by operand split.
//
// The contract of K13 (conv1x1.hip, mtr_conv1x1_bias_act_pre) for f32 tensors, per image b:
//
//   v[b, k, p] = act_in(x[b, k, p] + in_bias[k])  (or x without a prologue), then v * gate[b, k] with a gate
//   y[b, m, p] = act(bias[m] + sum_k w[m, k] * v[b, k, p]) (+ residual[b, m, p])
//
// but the f32 product is evaluated on v_mfma_f32_16x16x32_bf16 (1/16 of the cycles per FLOP of the f32-input
// MFMA K13 runs on).  An f32 value is exactly the sum of three bf16 values (8 + 8 + 8 significant bits, f32's
// exponent range):
//   a0 = bf16_rn(a), a1 = bf16_rn(a - a0), a2 = bf16_rn(a - a0 - a1)      (the subtractions are exact in f32)
// with |a1| <= 2^-8 |a| and |a2| <= 2^-16 |a|.  Of the nine cross products of w = w0 + w1 + w2 and v = v0 + v1 + v2
// the six with piece indices summing to at most 2 carry everything above 2^-23 |w v|; the other three are
// dropped.  Per 32-k step and 16 x 16 output tile the six MFMAs accumulate into ONE f32 accumulator in one fixed
// order, smallest first:
//   (w2, v0), (w0, v2), (w1, v1), (w1, v0), (w0, v1), (w0, v0)
// and the k steps run in k order: no split-K, no atomics, the same inputs give the same bits whatever the tile.
// The results are NOT the bits of K13 (another summation order, other roundings); against fp64 they pass K13's
// bound.
//
// The weight arrives split (kernels.pack_conv1x1_split_weight): [3][M][Kp] bf16, Kp = K rounded up to 32, the
// tail zero.  x is split on the VALU on its way from global memory into LDS, after the prologue and the gate
// (v_cvt_pk_bf16_f32 rounds to nearest even): once per element per workgroup.  Its k tail and the columns past
// B * HW are zeros by predicate.
//
// Non-finite inputs: x - bf16(x) of an infinity is NaN, so a column that holds an infinity (or a value that
// rounds to one in bf16, |x| >= 2^127 * (2 - 2^-8)) gives NaN where K13 gives an infinity.  Finite inputs below
// 2^127 behave as described.
//
// Geometry.  The product is computed transposed, Y_b^T = V_b^T W^T: the MFMA's A operand is a 16 (positions) x 32
// (k) slice of V^T, its B operand a 32 (k) x 16 (channels) slice of W^T, so a lane ends with four CONSECUTIVE
// positions of one channel in the four accumulator registers: one 16-byte store, the epilogue applied in registers.
// A workgroup of four waves owns 64 columns (over image and position jointly, as K13) and 64 MT channels, MT = 1 .. 4:
// all of M <= 256 where the grid still fills the chip, so x is read once; fewer channels per workgroup where the
// columns alone give too few workgroups (8 x 8 maps), the re-reads of x then come from L2.  M above 256 is walked in
// blocks by the grid.  Wave w owns the 16-channel tiles w, w + 4, .. of the block (M = 160: 3, 3, 2, 2 tiles) and all
// four 16-column tiles: 4 MT accumulators, enough independent MFMAs between two into the same accumulator.
//   * x: k-tiles of 32, global -> a ring of three tiles in registers (a load has two tiles of MFMA time to arrive) ->
//     split -> LDS, two buffers.  Each thread holds four columns x two k: per column and piece one 4-byte LDS write
//     of a bf16 pair.  LDS image per piece: [column][32 k] bf16, 64-byte rows, so the A fragment (8 consecutive k of
//     one column) is one ds_read_b128; the four 16-byte slots of a row are XOR-swizzled with (-(column >> 2)) & 3,
//     which spreads each of ds_read_b128's lane groups over all 16 slots of the 256-byte bank row.
//   * w: the B fragment is 16 contiguous bytes of a packed row, read straight from L2 (the whole packed weight of
//     the largest project is under 1 MB), each by the one wave that needs it, one k step ahead.
#include <type_traits>

#include "common.h"

namespace mtr {

typedef float sp_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 sp_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kSpBN = 64;                  // columns per workgroup
constexpr int kSpBK = 32;                  // k per step: one v_mfma_f32_16x16x32_bf16
constexpr int kSpWaves = 4;
constexpr int kSpNT = 64 * kSpWaves;
constexpr int kSpPiece = kSpBN * kSpBK * 2;    // bytes of one piece of one x stage
constexpr int kSpStage = 3 * kSpPiece;         // 12 KiB
constexpr int kSpMaxMT = 4;

// byte offset of (column c, 16-byte slot q = k / 8) inside one piece of a stage
__device__ __forceinline__ int sp_slot(int c, int q) { return c * 64 + ((q ^ (-(c >> 2))) & 3) * 16; }

template <int MT, int PRE, bool GATE>
__global__ __launch_bounds__(kSpNT) void conv1x1_split_kernel(
    const float* __restrict__ x, const uint4* __restrict__ ws, const float* __restrict__ bias,
    const float* __restrict__ in_bias, const float* __restrict__ gate, const float* __restrict__ residual,
    float* __restrict__ y, int act, int M, int K, int Kp, int HW, int n_total, FastDiv by_hw) {
  __shared__ __attribute__((aligned(16))) unsigned char xs[2 * kSpStage];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int n0 = blockIdx.x * kSpBN;
  const int mt0 = blockIdx.y * (kSpWaves * MT) + wave;  // this wave's tiles: mt0 + 4 i

  // ---- x loader: columns 4 cg .. 4 cg + 3 of the tile, rows k0 + 2 kp, k0 + 2 kp + 1.  Every load is issued
  // unconditionally from a clamped, valid address and selected against zero afterwards: a branch around a load makes
  // the compiler wait for everything in flight where the branch joins
  const int cg = tid & 15, kp = tid >> 4;
  const int xcol = n0 + cg * 4;
  const bool xcol_ok = xcol < n_total;
  const unsigned xb = xcol_ok ? fastdiv((unsigned)xcol, by_hw) : 0u;
  const float* xsrc = x + (long long)xb * K * HW + (xcol_ok ? xcol - (int)xb * HW : 0);
  const float* gsrc = GATE ? gate + (long long)xb * K : nullptr;
  // (column c = 4 cg + i: c >> 2 = cg) the 4-byte slot of this thread's k pair in column 4 cg, + 64 i per column
  const int xdst = sp_slot(cg * 4, kp >> 2) + (kp & 3) * 4;

  // A ring of three k-tiles in registers (raw f32, 8 per tile): tile t + 3 is requested before tile t is multiplied
  // and tile t + 1, requested two whole tiles earlier, is finished (prologue, gate, split) and written to LDS behind
  // tile t's MFMAs: a load has two tiles of MFMA time to arrive.  The slot is a compile-time index (the k loop is
  // unrolled by three): a ring indexed at run time would live in scratch.
  float4 xr[3][2];
  float xbi[3][2], xg[3][2];
  bool xr_ok[3];
  auto load_x = [&](auto slot, int tile) {
    constexpr int S = decltype(slot)::value;
    const int k0 = tile * kSpBK;
    xr_ok[S] = xcol_ok && k0 + 2 * kp < K;      // (K % 4 == 0: a pair never straddles K; a tile past the last: zeros)
    const int k = min(k0 + 2 * kp, K - 2);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      xr[S][r] = *reinterpret_cast<const float4*>(xsrc + (long long)(k + r) * HW);
      if constexpr (PRE >= 0) xbi[S][r] = in_bias[k + r]; else xbi[S][r] = 0.0f;
      if constexpr (GATE) xg[S][r] = gsrc[k + r];
    }
  };
  auto store_x = [&](auto slot, int buf) {
    constexpr int S = decltype(slot)::value;
    unsigned char* d = xs + buf * kSpStage + xdst;
    float v[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const float t[4] = {xr[S][r].x, xr[S][r].y, xr[S][r].z, xr[S][r].w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float e = input_prologue<PRE>(t[i], xbi[S][r]);
        if constexpr (GATE) e *= xg[S][r];  // the squeeze-excite gate: x * g rounded to f32 as torch does, then split
        v[r][i] = xr_ok[S] ? e : 0.0f;      // a column past B * HW or a k past K: zeros, whatever the prologue
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned pk[3];
      split_bf16x3_pairs(v[0][i], v[1][i], pk);
#pragma unroll
      for (int p = 0; p < 3; ++p) *reinterpret_cast<unsigned*>(d + p * kSpPiece + i * 64) = pk[p];
    }
  };

  // ---- w fragments: row min(m, M - 1) (a row past M, or a whole tile past it, feeds only channels that are never
  // stored; the waves of a workgroup run side by side, so such a tile costs no time), 16 bytes at k0 + 8 fq of each piece
  const uint4* wsrc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = min((mt0 + kSpWaves * i) * 16 + fr, M - 1);
    wsrc[i] = ws + ((long long)m * Kp >> 3) + fq;
  }
  const long long wpiece = (long long)M * Kp >> 3;  // uint4 per piece
  uint4 wn[MT][3];
  auto load_w = [&](int k0) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) wn[i][p] = wsrc[i][p * wpiece + (k0 >> 3)];
  };

  sp_f32x4 acc[MT][4];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = sp_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

  const int n_tiles = (K + kSpBK - 1) / kSpBK;
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  using S2 = std::integral_constant<int, 2>;
  load_x(S0{}, 0);
  load_x(S1{}, 1);
  load_x(S2{}, 2);
  load_w(0);
  store_x(S0{}, 0);
  __syncthreads();
  // one k-tile: `slot` = t % 3 held tile t (written to LDS one pass ago) and takes tile t + 3; `next` = (t + 1) % 3
  auto step = [&](auto slot, auto next, int t) {
    const int buf = t & 1;
    uint4 wc[MT][3];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int p = 0; p < 3; ++p) wc[i][p] = wn[i][p];
    // Unconditional, like the LDS write below (past the last tile: clamped addresses, zeros into the buffer nobody
    // reads any more): behind a branch the compiler sinks the x loads next to their use or copies the loaded registers
    // where the branch joins, and either waits for them in front of the MFMAs; the scheduling barrier keeps the x
    // loads in front of the MFMAs at the machine level too
    load_x(slot, t + 3);
    __builtin_amdgcn_sched_barrier(0);
    load_w(min(t + 1, n_tiles - 1) * kSpBK);
    sp_bf16x8 xa[4][3];
    const unsigned char* xsb = xs + buf * kSpStage;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        xa[j][p] = *reinterpret_cast<const sp_bf16x8*>(xsb + p * kSpPiece + sp_slot(j * 16 + fr, fq));
    // the six products, smallest first; (w piece, x piece)
    constexpr int kWp[6] = {2, 0, 1, 1, 0, 0}, kXp[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
    for (int s = 0; s < 6; ++s)
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const sp_bf16x8 wb = __builtin_bit_cast(sp_bf16x8, wc[i][kWp[s]]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[j][kXp[s]], wb, acc[i][j], 0, 0, 0);
      }
    store_x(next, buf ^ 1);  // tile t + 1 into the other buffer: last read before the previous barrier
    __syncthreads();
  };
  int t = 0;
  for (; t + 3 <= n_tiles; t += 3) {  // (no exit from inside a group: one copy of the accumulators, one epilogue)
    step(S0{}, S1{}, t);
    step(S1{}, S2{}, t + 1);
    step(S2{}, S0{}, t + 2);
  }
  if (t < n_tiles) {
    step(S0{}, S1{}, t);
    if (t + 1 < n_tiles) step(S1{}, S2{}, t + 1);
  }

  // ---- epilogue: lane holds channel 16 mt + fr, positions n0 + 16 j + 4 fq + 0 .. 3
  auto epilogue = [&](auto tag) {
    constexpr int ACT = decltype(tag)::value;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = (mt0 + kSpWaves * i) * 16 + fr;
      if (m >= M) continue;
      const float bm = bias[m];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = n0 + j * 16 + fq * 4;
        if (col >= n_total) continue;
        const unsigned b = fastdiv((unsigned)col, by_hw);
        const long long off = ((long long)b * M + m) * HW + (col - (int)b * HW);
        epilogue_store4<ACT>(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3], bm, residual, y, off);
      }
    }
  };
  // (a run-time code: the activation is a few instructions of the epilogue, not worth 4 x the kernels)
  with_act(act, epilogue);
}

// 16-channel tiles per wave: all of the layer's (at most 4: 256 channels per workgroup) while the grid has a
// workgroup per CU, fewer otherwise.  A pure function of the shape; the bits do not depend on it.
static int split_tiles_per_wave(int M, long long n_total) {
  const int n_mt = (M + 15) / 16;
  const long long gx = (n_total + kSpBN - 1) / kSpBN;
  int mt = (n_mt + kSpWaves - 1) / kSpWaves;
  if (mt > kSpMaxMT) mt = kSpMaxMT;
  while (mt > 1 && gx * ((n_mt + kSpWaves * mt - 1) / (kSpWaves * mt)) < 256) --mt;
  return mt;
}

// One K20 launch's arguments, as the entry point has checked them
struct SplitArgs {
  const float* x;
  const void* ws;
  const float *bias, *in_bias, *gate, *residual;
  float* y;
  int act, in_act, M, K, HW;
  long long n_total;
  hipStream_t stream;
};

template <int MT>
static int launch_split(const SplitArgs& a) {
  const int Kp = (a.K + 31) / 32 * 32;
  const int n_mt = (a.M + 15) / 16;
  const long long gx = (a.n_total + kSpBN - 1) / kSpBN, gy = (n_mt + kSpWaves * MT - 1) / (kSpWaves * MT);
  if (gx > 0x7fffffffLL || gy > 65535) return MTR_E_SHAPE;
  return dispatch_pre(a.in_bias, a.in_act, [&](auto pre) {
    const auto go = [&](auto kern) -> int {
      MTR_CLEAR_STALE();
      hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(kSpNT), 0, a.stream, a.x, (const uint4*)a.ws,
                         a.bias, a.in_bias, a.gate, a.residual, a.y, a.act, a.M, a.K, Kp, a.HW, (int)a.n_total,
                         make_fastdiv((unsigned)a.HW));
      MTR_CHECK_LAUNCH();
      return MTR_OK;
    };
    constexpr int PRE = decltype(pre)::value;
    return a.gate ? go(conv1x1_split_kernel<MT, PRE, true>) : go(conv1x1_split_kernel<MT, PRE, false>);
  });
}

}  // namespace mtr

extern "C" int mtr_conv1x1_split_supported(long long B, int M, int K, int HW) {
  return mtr::conv1x1_shape_check(B, M, K, HW, 4);  // 16-byte groups: four positions of x / y / residual
}

extern "C" int mtr_conv1x1_bias_act_split(const void* x, const void* w_split, const float* bias,
                                          const float* in_bias, int in_act, const float* gate,
                                          const void* residual, int act, long long B, int M, int K, int HW,
                                          void* y, mtr_stream_t stream) {
  if (!x || !w_split || !bias || !y) return MTR_E_NULL;
  const int e = mtr::conv1x1_shape_check(B, M, K, HW, 4);
  if (e != MTR_OK) return e;
  if (act < mtr::kActNone || act > mtr::kActHardswish) return MTR_E_PARAM;
  if (in_act < mtr::kActNone || in_act > mtr::kActHardswish) return MTR_E_PARAM;
  if (!in_bias && in_act != mtr::kActNone) return MTR_E_PARAM;  // an input activation belongs to an input bias
  if (((uintptr_t)x % 16) || ((uintptr_t)w_split % 16) || ((uintptr_t)y % 16) || ((uintptr_t)residual % 16) ||
      ((uintptr_t)in_bias % 4))
    return MTR_E_ALIGN;
  // y is written while x and the residual of other columns are still read: no overlap at all
  const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (size_t)B * M * HW * 4;
  const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (size_t)B * K * HW * 4;
  const uintptr_t r0 = (uintptr_t)residual, r1 = r0 + (size_t)B * M * HW * 4;
  if (x == y || (residual && residual == x)) return MTR_E_PARAM;
  if (B > 0 && ((x0 < y1 && y0 < x1) || (residual && r0 < y1 && y0 < r1))) return MTR_E_PARAM;
  if (B == 0) return MTR_OK;
  const mtr::SplitArgs a = {(const float*)x, w_split, bias, in_bias, gate, (const float*)residual, (float*)y,
                             act, in_act, M, K, HW, B * HW, (hipStream_t)stream};
  switch (mtr::split_tiles_per_wave(M, a.n_total)) {
    case 1: return mtr::launch_split<1>(a);
    case 2: return mtr::launch_split<2>(a);
    case 3: return mtr::launch_split<3>(a);
    default: return mtr::launch_split<4>(a);
  }
}
