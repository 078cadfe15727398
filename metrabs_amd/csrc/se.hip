// K12: the squeeze-excite gate of an MBConv block in one launch.
//
// Not part of the reference's hot path (like K10 / K11): the SE tail of the backbone's inference copy
// (backbones.fold_batchnorm(fused_epilogue=True)).  PyTorch-ROCm runs it as six kernels per block --
// fc1 (a rocBLAS GEMM on [B, C, 1, 1]), "+ b1", the activation, fc2, "+ b2", the gate function -- on
// a few MFLOP each, so launch boundaries and near-empty GEMM tiles are what it costs.  Here:
//
//   gate[b, c] = gate_fn(b2[c] + sum_s W2[c, s] * act(b1[s] + sum_k W1[s, k] * mean[b, k]))
//
// from the [B, C] f32 channel mean K10 / K11 already emit.  One workgroup of 16 waves = IMG images x
// a slice of CS output channels.  Every workgroup computes the whole hidden vector of its images (fc1
// reads W1 once for IMG images: the redundancy across slices is a re-read of W1 from L2, not from HBM),
// keeps it in LDS and computes fc2 for its slice.  Phase 1: one wave per block of 4 hidden rows (2 at
// IMG = 8), two passes' loads in flight (S = 64: every wave owns one block, so all of W1 is requested by
// 16 waves in three rounds instead of by 4 waves in 24 dependent ones), lanes strided over the
// channels in 16-byte vectors, the mean tile of the images from LDS; the per-lane partial sums are
// summed by a fixed xor butterfly.  Phase 2: one thread per (group of IPT images, output channel), the
// hidden vector broadcast from LDS; with the transposed weight W2^T [S][C] (mtr_se_gate_opts, layout
// MTR_SE_W2_SC) a wave's load is 256 contiguous bytes instead of 64 cache lines.  The summation order
// of an image never depends on the configuration, on its slot in the workgroup, on B or on the layout
// of W2: per lane k = 4 lane + 256 j + (0..3) ascending, the butterfly, then s = 0, 1, 2, ... -- the
// order of this kernel's first version, whose bits it returns.  No atomics.
#include "common.h"

namespace mtr {

enum SeGate { kGateSigmoid = 0, kGateHardsigmoid = 1 };

constexpr int kSeThreads = 1024;
constexpr int kSeImg = 4;   // images per workgroup the argument rules are stated for (mtr_se_gate)

// (IMG images per workgroup, IPT images per phase-2 thread): CS = 1024 IPT / IMG channels per slice
template <int IMG, int IPT, bool W2T>
__global__ __launch_bounds__(kSeThreads) void se_gate_kernel(const float* __restrict__ mean,
                                                             const float* __restrict__ w1,
                                                             const float* __restrict__ b1,
                                                             const float* __restrict__ w2,
                                                             const float* __restrict__ b2, int act,
                                                             int gate_fn, int B, int C, int S,
                                                             float* __restrict__ gate) {
  constexpr int kSeRows = IMG <= 4 ? 4 : 2;    // fc1 rows per wave pass: at most 16 sums per lane
  constexpr int kSeUnroll = IMG <= 4 ? 2 : 1;  // fc1 passes whose loads are in flight together
  static_assert(IMG % IPT == 0 && kSeThreads % (IMG / IPT) == 0, "thread mapping");
  constexpr int CS = kSeThreads / (IMG / IPT);
  extern __shared__ float4 se_lds[];
  const int C4 = C >> 2;
  float4* m_tile = se_lds;                                   // [IMG][C / 4]
  float* hid = reinterpret_cast<float*>(se_lds + IMG * C4);  // [IMG][S]
  const int b0 = blockIdx.y * IMG;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the means of this workgroup's images (rows past B: zeros, never stored)
  for (int i = tid; i < IMG * C4; i += kSeThreads) {
    const int img = i / C4, c4 = i - img * C4;
    m_tile[i] = b0 + img < B ? reinterpret_cast<const float4*>(mean)[(long long)(b0 + img) * C4 + c4]
                             : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  __syncthreads();

  // phase 1: hid[i][s] = act(b1[s] + W1[s, :] . mean[i, :])
  const int n_blocks = (S + kSeRows - 1) / kSeRows;
  for (int blk = wave; blk < n_blocks; blk += kSeThreads / 64) {
    const float4* wrow[kSeRows];
#pragma unroll
    for (int r = 0; r < kSeRows; ++r) {
      const int s = min(blk * kSeRows + r, S - 1);  // rows past S recompute row S - 1, never stored
      wrow[r] = reinterpret_cast<const float4*>(w1 + (long long)s * C);
    }
    float acc[kSeRows][IMG];
#pragma unroll
    for (int r = 0; r < kSeRows; ++r)
#pragma unroll
      for (int i = 0; i < IMG; ++i) acc[r][i] = 0.0f;
    // kSeUnroll passes' W1 loads are issued before any of them is used; a pass wholly past C is not
    // loaded (a wave-uniform test), a partly dead one loads its last vector again and multiplies by zeros
    for (int cb = 0; cb < C4; cb += 64 * kSeUnroll) {
      float4 w[kSeUnroll][kSeRows];
#pragma unroll
      for (int u = 0; u < kSeUnroll; ++u) {
        if (cb + 64 * u < C4) {
#pragma unroll
          for (int r = 0; r < kSeRows; ++r) w[u][r] = wrow[r][min(cb + 64 * u + lane, C4 - 1)];
        } else {
#pragma unroll
          for (int r = 0; r < kSeRows; ++r) w[u][r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
      }
#pragma unroll
      for (int u = 0; u < kSeUnroll; ++u) {
        const int c4 = cb + 64 * u + lane;
        const bool live = c4 < C4;  // (a select, not a branch: a branch lets the compiler sink the loads)
#pragma unroll
        for (int i = 0; i < IMG; ++i) {
          const float4 v = m_tile[i * C4 + min(c4, C4 - 1)];
          const float4 m = live ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // a dead pass adds exact zeros
#pragma unroll
          for (int r = 0; r < kSeRows; ++r) {
            float a = acc[r][i];
            a = fmaf(w[u][r].x, m.x, a);
            a = fmaf(w[u][r].y, m.y, a);
            a = fmaf(w[u][r].z, m.z, a);
            a = fmaf(w[u][r].w, m.w, a);
            acc[r][i] = a;
          }
        }
      }
    }
    // the butterfly leaves every sum in every lane: lane r * IMG + i keeps, finishes and stores hid[i][s0 + r]
    float mine = 0.0f;
#pragma unroll
    for (int r = 0; r < kSeRows; ++r)
#pragma unroll
      for (int i = 0; i < IMG; ++i) {
        float v = acc[r][i];
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
        mine = lane == r * IMG + i ? v : mine;
      }
    const int s = blk * kSeRows + lane / IMG;
    if (lane < kSeRows * IMG && s < S) {
      const float h = mine + b1[s];
      float a = h;
      if (act == kActRelu) a = activate<kActRelu>(h);
      else if (act == kActSilu) a = activate<kActSilu>(h);
      else if (act == kActHardswish) a = activate<kActHardswish>(h);
      hid[(lane % IMG) * S + s] = a;
    }
  }
  __syncthreads();

  // phase 2: gate[i][c] = gate_fn(b2[c] + W2[c, :] . hid[i, :]) for this workgroup's channel slice
  const int isub = tid / CS;  // wave-uniform: CS is a multiple of 64
  const int c = blockIdx.x * CS + (tid - isub * CS);
  if (c >= C) return;
  const float* hrow = hid + isub * IPT * S;
  const float* wsrc = W2T ? w2 + c : w2 + (long long)c * S;
  const long long wstep = W2T ? C : 1;
  float z[IPT];
#pragma unroll
  for (int i = 0; i < IPT; ++i) z[i] = 0.0f;
  // (unrolled: sixteen independent loads in flight, not one load's latency per term)
#pragma unroll 16
  for (int s = 0; s < S; ++s) {
    const float w = wsrc[s * wstep];
#pragma unroll
    for (int i = 0; i < IPT; ++i) z[i] = fmaf(w, hrow[i * S + s], z[i]);
  }
  const float bias = b2[c];
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const int b = b0 + isub * IPT + i;
    if (b >= B) break;
    const float x = z[i] + bias;
    float g;
    if (gate_fn == kGateSigmoid) g = 1.0f / (1.0f + expf(-x));
    else g = fminf(fmaxf(x + 3.0f, 0.0f), 6.0f) / 6.0f;  // torch.nn.Hardsigmoid
    gate[(long long)b * C + c] = g;
  }
}

// The configurations (IMG, IPT): every one gives the same bits, so the choice may depend on B.
//   0 (4, 1): 4 images x 256 channels      1 (4, 4): 4 images x 1024 channels
//   2 (8, 2): 8 images x 256 channels      3 (2, 1): 2 images x 512 channels
constexpr int kSeConfigs = 4;

inline size_t se_lds_bytes(int img, int C, int S) { return (size_t)img * ((size_t)C + S) * sizeof(float); }

// A pure function of (B, C, S); see DESIGN.md section 15 for the measurements behind it.  Two images per
// workgroup are fastest (the 32 sums of a wave's butterfly and the mean tile halve) as long as the re-reads of
// W1 they cost -- once per workgroup -- stay in the tens of megabytes; past that, the fewest workgroups.
inline int se_pick_config(int B, int C, int S) {
  const long long groups2 = ((long long)B + 1) / 2, slices2 = (C + 511) / 512;
  const long long w1_reread = groups2 * slices2 * S * C * 4;
  if (groups2 <= 65535 && w1_reread <= 64ll << 20) return 3;
  return 1;
}

template <int IMG, int IPT, bool W2T>
static int launch_se_gate(const float* mean, const float* w1, const float* b1, const float* w2,
                          const float* b2, int act, int gate_fn, int B, int C, int S, float* gate,
                          hipStream_t stream) {
  constexpr int CS = kSeThreads / (IMG / IPT);
  const size_t lds = se_lds_bytes(IMG, C, S);
  const int gy = (B + IMG - 1) / IMG;
  if (gy > 65535 || lds > 160 * 1024) return MTR_E_SHAPE;
  const dim3 grid((C + CS - 1) / CS, gy), block(kSeThreads);
  if (lds > 64 * 1024) {
    const int e = allow_dynamic_lds((const void*)se_gate_kernel<IMG, IPT, W2T>, lds);
    if (e != MTR_OK) return e;
  }
  MTR_CLEAR_STALE();
  hipLaunchKernelGGL((se_gate_kernel<IMG, IPT, W2T>), grid, block, lds, stream, mean, w1, b1, w2, b2, act,
                     gate_fn, B, C, S, gate);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

template <bool W2T>
static int launch_se_gate_cfg(int config, const float* mean, const float* w1, const float* b1,
                              const float* w2, const float* b2, int act, int gate_fn, int B, int C, int S,
                              float* gate, hipStream_t stream) {
  switch (config) {
    case 0: return launch_se_gate<4, 1, W2T>(mean, w1, b1, w2, b2, act, gate_fn, B, C, S, gate, stream);
    case 1: return launch_se_gate<4, 4, W2T>(mean, w1, b1, w2, b2, act, gate_fn, B, C, S, gate, stream);
    case 2: return launch_se_gate<8, 2, W2T>(mean, w1, b1, w2, b2, act, gate_fn, B, C, S, gate, stream);
    default: return launch_se_gate<2, 1, W2T>(mean, w1, b1, w2, b2, act, gate_fn, B, C, S, gate, stream);
  }
}

}  // namespace mtr

extern "C" int mtr_se_gate_opts(const float* mean, const float* w1, const float* b1, const float* w2,
                                const float* b2, int act, int gate_fn, int B, int C, int S, float* gate,
                                mtr_stream_t stream, int w2_layout, int config) {
  if (!mean || !w1 || !b1 || !w2 || !b2 || !gate) return MTR_E_NULL;
  if (B < 0 || C <= 0 || S <= 0 || C % 4 || (B + mtr::kSeImg - 1) / mtr::kSeImg > 65535) return MTR_E_SHAPE;
  // the LDS tile: IMG mean rows + IMG hidden rows within 160 KiB
  if ((long long)mtr::kSeImg * (C + S) * 4 > 160 * 1024) return MTR_E_SHAPE;
  if (((uintptr_t)mean % 16) || ((uintptr_t)w1 % 16)) return MTR_E_ALIGN;
  if (gate_fn != mtr::kGateSigmoid && gate_fn != mtr::kGateHardsigmoid) return MTR_E_PARAM;
  if (act < mtr::kActNone || act > mtr::kActHardswish) return MTR_E_PARAM;
  if (w2_layout != MTR_SE_W2_CS && w2_layout != MTR_SE_W2_SC) return MTR_E_PARAM;
  if (config < -1 || config >= mtr::kSeConfigs) return MTR_E_PARAM;
  if (B == 0) return MTR_OK;
  if (config < 0) config = mtr::se_pick_config(B, C, S);
  hipStream_t s = (hipStream_t)stream;
  if (w2_layout == MTR_SE_W2_SC)
    return mtr::launch_se_gate_cfg<true>(config, mean, w1, b1, w2, b2, act, gate_fn, B, C, S, gate, s);
  return mtr::launch_se_gate_cfg<false>(config, mean, w1, b1, w2, b2, act, gate_fn, B, C, S, gate, s);
}

extern "C" int mtr_se_gate(const float* mean, const float* w1, const float* b1, const float* w2,
                           const float* b2, int act, int gate_fn, int B, int C, int S, float* gate,
                           mtr_stream_t stream) {
  return mtr_se_gate_opts(mean, w1, b1, w2, b2, act, gate_fn, B, C, S, gate, stream, MTR_SE_W2_CS, -1);
}
