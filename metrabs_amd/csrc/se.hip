// K12: the squeeze-excite gate of an MBConv block in one launch.
//
// Not part of the reference's hot path (like K10 / K11): the SE tail of the backbone's inference copy
// (backbones.fold_batchnorm(fused_epilogue=True)).  PyTorch-ROCm runs it as six kernels per block --
// fc1 (a rocBLAS GEMM on [B, C, 1, 1]), "+ b1", the activation, fc2, "+ b2", the gate function -- on
// a few MFLOP each, so launch boundaries and near-empty GEMM tiles are what it costs.  Here:
//
//   gate[b, c] = gate_fn(b2[c] + sum_s W2[c, s] * act(b1[s] + sum_k W1[s, k] * mean[b, k]))
//
// from the [B, C] f32 channel mean K10 / K11 already emit.  One workgroup = IMG images x a slice of
// 256 output channels.  Every workgroup computes the whole hidden vector of its images (fc1 reads
// W1 once for IMG images: the redundancy across slices is a re-read of W1 from L2, not from HBM),
// keeps it in LDS and computes fc2 for its slice.  Phase 1: one wave per block of R hidden rows,
// lanes strided over the channels in 16-byte vectors, the mean tile of the images from LDS; the
// per-lane partial sums are summed by a fixed xor butterfly.  Phase 2: one lane per output channel,
// the hidden vector broadcast from LDS.  Fixed summation order everywhere, no atomics: the same
// inputs give the same bits.
#include "common.h"

namespace mtr {

enum SeGate { kGateSigmoid = 0, kGateHardsigmoid = 1 };

constexpr int kSeThreads = 256;
constexpr int kSeImg = 4;  // images per workgroup
constexpr int kSeRows = 4; // fc1 rows per wave pass
constexpr int kSeUnroll = 4;  // fc1 passes whose loads are in flight together

template <int ACT, int GATE>
__global__ __launch_bounds__(kSeThreads) void se_gate_kernel(const float* __restrict__ mean,
                                                             const float* __restrict__ w1,
                                                             const float* __restrict__ b1,
                                                             const float* __restrict__ w2,
                                                             const float* __restrict__ b2, int B,
                                                             int C, int S, float* __restrict__ gate) {
  extern __shared__ float4 se_lds[];
  const int C4 = C >> 2;
  float4* m_tile = se_lds;                                    // [IMG][C / 4]
  float* hid = reinterpret_cast<float*>(se_lds + kSeImg * C4);  // [IMG][S]
  const int b0 = blockIdx.y * kSeImg;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // the means of this workgroup's images (rows past B: zeros, never stored)
  for (int i = tid; i < kSeImg * C4; i += kSeThreads) {
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
    float acc[kSeRows][kSeImg];
#pragma unroll
    for (int r = 0; r < kSeRows; ++r)
#pragma unroll
      for (int i = 0; i < kSeImg; ++i) acc[r][i] = 0.0f;
    // kSeUnroll passes' W1 loads are issued before any of them is used: the loop is bound by load
    // latency, not by issue (one workgroup per CU at the bench shapes)
    for (int c0 = lane; c0 < C4; c0 += 64 * kSeUnroll) {
      float4 w[kSeUnroll][kSeRows];
#pragma unroll
      for (int u = 0; u < kSeUnroll; ++u)
#pragma unroll
        for (int r = 0; r < kSeRows; ++r)
          w[u][r] = wrow[r][min(c0 + 64 * u, C4 - 1)];  // (passes past C4: loaded, multiplied by zeros)
#pragma unroll
      for (int u = 0; u < kSeUnroll; ++u) {
        const int c4 = c0 + 64 * u;
        const bool live = c4 < C4;  // (a select, not a branch: a branch lets the compiler sink the loads)
        float4 m[kSeImg];
#pragma unroll
        for (int i = 0; i < kSeImg; ++i) {
          const float4 v = m_tile[i * C4 + min(c4, C4 - 1)];
          m[i] = live ? v : make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // a dead pass adds exact zeros
        }
#pragma unroll
        for (int r = 0; r < kSeRows; ++r)
#pragma unroll
          for (int i = 0; i < kSeImg; ++i) {
            float a = acc[r][i];
            a = fmaf(w[u][r].x, m[i].x, a);
            a = fmaf(w[u][r].y, m[i].y, a);
            a = fmaf(w[u][r].z, m[i].z, a);
            a = fmaf(w[u][r].w, m[i].w, a);
            acc[r][i] = a;
          }
      }
    }
#pragma unroll
    for (int r = 0; r < kSeRows; ++r)
#pragma unroll
      for (int i = 0; i < kSeImg; ++i) {
        float v = acc[r][i];
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
        acc[r][i] = v;  // the same value in every lane
      }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < kSeRows; ++r) {
        const int s = blk * kSeRows + r;
        if (s < S) {
#pragma unroll
          for (int i = 0; i < kSeImg; ++i) hid[i * S + s] = activate<ACT>(acc[r][i] + b1[s]);
        }
      }
    }
  }
  __syncthreads();

  // phase 2: gate[i][c] = gate_fn(b2[c] + W2[c, :] . hid[i, :]) for this workgroup's channel slice
  const int c = blockIdx.x * kSeThreads + tid;
  if (c >= C) return;
  const float* w2row = w2 + (long long)c * S;
  float z[kSeImg];
#pragma unroll
  for (int i = 0; i < kSeImg; ++i) z[i] = 0.0f;
  // (unrolled: sixteen independent loads of the row in flight, not one load's latency per term)
#pragma unroll 16
  for (int s = 0; s < S; ++s) {
    const float w = w2row[s];
#pragma unroll
    for (int i = 0; i < kSeImg; ++i) z[i] = fmaf(w, hid[i * S + s], z[i]);
  }
  const float bias = b2[c];
#pragma unroll
  for (int i = 0; i < kSeImg; ++i) {
    if (b0 + i >= B) break;
    const float x = z[i] + bias;
    float g;
    if constexpr (GATE == kGateSigmoid) g = 1.0f / (1.0f + expf(-x));
    else g = fminf(fmaxf(x + 3.0f, 0.0f), 6.0f) / 6.0f;  // torch.nn.Hardsigmoid
    gate[(long long)(b0 + i) * C + c] = g;
  }
}

template <int ACT>
static int launch_se_gate(const float* mean, const float* w1, const float* b1, const float* w2,
                          const float* b2, int gate_fn, int B, int C, int S, float* gate,
                          hipStream_t stream) {
  const size_t lds = (size_t)kSeImg * C * sizeof(float) + (size_t)kSeImg * S * sizeof(float);
  const dim3 grid((C + kSeThreads - 1) / kSeThreads, (B + kSeImg - 1) / kSeImg), block(kSeThreads);
  const void* kern = gate_fn == kGateSigmoid ? (const void*)se_gate_kernel<ACT, kGateSigmoid>
                                             : (const void*)se_gate_kernel<ACT, kGateHardsigmoid>;
  if (lds > 64 * 1024) {
    const int e = allow_dynamic_lds(kern, lds);
    if (e != MTR_OK) return e;
  }
  MTR_CLEAR_STALE();
  if (gate_fn == kGateSigmoid)
    hipLaunchKernelGGL((se_gate_kernel<ACT, kGateSigmoid>), grid, block, lds, stream, mean, w1, b1, w2, b2,
                       B, C, S, gate);
  else
    hipLaunchKernelGGL((se_gate_kernel<ACT, kGateHardsigmoid>), grid, block, lds, stream, mean, w1, b1, w2,
                       b2, B, C, S, gate);
  MTR_CHECK_LAUNCH();
  return MTR_OK;
}

}  // namespace mtr

extern "C" int mtr_se_gate(const float* mean, const float* w1, const float* b1, const float* w2,
                           const float* b2, int act, int gate_fn, int B, int C, int S, float* gate,
                           mtr_stream_t stream) {
  if (!mean || !w1 || !b1 || !w2 || !b2 || !gate) return MTR_E_NULL;
  if (B < 0 || C <= 0 || S <= 0 || C % 4 || (B + mtr::kSeImg - 1) / mtr::kSeImg > 65535) return MTR_E_SHAPE;
  // the LDS tile: IMG mean rows + IMG hidden rows within 160 KiB
  if ((long long)mtr::kSeImg * (C + S) * 4 > 160 * 1024) return MTR_E_SHAPE;
  if (((uintptr_t)mean % 16) || ((uintptr_t)w1 % 16)) return MTR_E_ALIGN;
  if (gate_fn != mtr::kGateSigmoid && gate_fn != mtr::kGateHardsigmoid) return MTR_E_PARAM;
  if (B == 0) return MTR_OK;
  hipStream_t s = (hipStream_t)stream;
  switch (act) {
    case mtr::kActNone: return mtr::launch_se_gate<mtr::kActNone>(mean, w1, b1, w2, b2, gate_fn, B, C, S, gate, s);
    case mtr::kActRelu: return mtr::launch_se_gate<mtr::kActRelu>(mean, w1, b1, w2, b2, gate_fn, B, C, S, gate, s);
    case mtr::kActSilu: return mtr::launch_se_gate<mtr::kActSilu>(mean, w1, b1, w2, b2, gate_fn, B, C, S, gate, s);
    case mtr::kActHardswish: return mtr::launch_se_gate<mtr::kActHardswish>(mean, w1, b1, w2, b2, gate_fn, B, C, S, gate, s);
    default: return MTR_E_PARAM;
  }
}
