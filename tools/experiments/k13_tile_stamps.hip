// Diagnostic build of K13's tall configurations (metrabs_amd/csrc/conv1x1.hip, conv1x1_kernel<w, 1, 1, 1, BK>) with
// in-kernel cycle stamps: where a k-tile's cycles go.  NOT part of the library; its run time means nothing (the
// stamps' fences forbid overlaps the real kernel has) -- read the SHARES.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/experiments/k13_tile_stamps.hip -o tools/experiments/_build/k13_tile_stamps
//   tools/experiments/_build/k13_tile_stamps            # on the GPU; prints one markdown table
//
// The loop is the library's, statement for statement (two LDS buffers, the next tile's global loads issued before
// the MFMAs, waited for and written to LDS after them, one barrier per tile), with a stamp between its parts:
//   issue   the next tile's global loads (address arithmetic + issue)
//   mfma    the tile's LDS fragment reads and MFMAs (until the last one has ISSUED: with one accumulator per wave
//           every MFMA waits for the one before, so only the last one's 64 cycles fall into the next part)
//   wait    s_waitcnt vmcnt(0): what is left of the global loads' latency
//   lds     the gate product and the LDS writes (W transposed, 4-byte writes), until they have landed
//   barrier s_barrier
// Per wave the five differences are summed over the k loop in scalar registers and written once, to a buffer of
// their own; the host averages over waves and prints shares.  A stamp costs about 40 cycles itself (measured as two
// stamps back to back, printed, and subtracted).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kPadX = 32, kPadW = 4;

__device__ __forceinline__ unsigned long long stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}

template <int WM, int BK>
__global__ __launch_bounds__(64 * WM) void k13_tall_stamped(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ gate, float* __restrict__ y,
                                                            int M, int K, int HW, int n_total,
                                                            unsigned long long* __restrict__ stamps) {
  constexpr int NT = 64 * WM, BM = 32 * WM, BN = 32;
  constexpr int LDX = BN + kPadX, LDW = BM + kPadW;
  constexpr int XROW4 = BN / 4, XPASS = NT / XROW4, XV = (BK + XPASS - 1) / XPASS;
  constexpr int WPASS = NT / (BK / 4), WV = (BM + WPASS - 1) / WPASS;
  __shared__ float xs[2][BK * LDX];
  __shared__ float ws[2][BK * LDW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int xn4 = tid % XROW4, xk0 = tid / XROW4;
  const int xcol = n0 + xn4 * 4;
  const bool xcol_ok = xcol < n_total;
  const int xb = xcol_ok ? xcol / HW : 0;
  const float* xsrc = x + (long long)xb * K * HW + (xcol - xb * HW);
  const float* gsrc = gate + (long long)xb * K;
  const int wk4 = tid % (BK / 4), wr0 = tid / (BK / 4);
  float4 xr[XV], wr[WV];
  float gr[XV];
#pragma unroll
  for (int v = 0; v < XV; ++v) gr[v] = 1.0f;
  auto load_tile = [&](int k0) {
#pragma unroll
    for (int v = 0; v < XV; ++v) {
      const int k = k0 + xk0 + v * XPASS;
      float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (xcol_ok && k < K && xk0 + v * XPASS < BK) {
        t = *reinterpret_cast<const float4*>(xsrc + (long long)k * HW);
        gr[v] = gsrc[k];
      }
      xr[v] = t;
    }
#pragma unroll
    for (int v = 0; v < WV; ++v) {
      const int m = m0 + wr0 + v * WPASS, k = k0 + wk4 * 4;
      float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (m < M && k < K && wr0 + v * WPASS < BM) t = *reinterpret_cast<const float4*>(w + (long long)m * K + k);
      wr[v] = t;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int v = 0; v < XV; ++v) {
      const int r = xk0 + v * XPASS;
      // (the gate product stands here, behind the wait, where the library build's scheduler leaves it: in
      // load_tile, as the source has it, the stamp's fence would pin the wait for x into "issue")
      const float4 t = make_float4(xr[v].x * gr[v], xr[v].y * gr[v], xr[v].z * gr[v], xr[v].w * gr[v]);
      if (r < BK) *reinterpret_cast<float4*>(&xs[buf][r * LDX + xn4 * 4]) = t;
    }
#pragma unroll
    for (int v = 0; v < WV; ++v) {
      const int r = wr0 + v * WPASS;
      if (r < BM) {
        float* d = &ws[buf][(wk4 * 4) * LDW + r];
        d[0] = wr[v].x; d[LDW] = wr[v].y; d[2 * LDW] = wr[v].z; d[3 * LDW] = wr[v].w;
      }
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const int half = lane >> 5, l32 = lane & 31;
  const int n_tiles = (K + BK - 1) / BK;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  unsigned long long sum[6] = {0, 0, 0, 0, 0, 0};
  for (int t = 0; t < n_tiles; ++t) {
    const int buf = t & 1;
    const unsigned long long t0 = stamp();
    const unsigned long long t0b = stamp();  // two stamps back to back: the stamp's own cost
    if (t + 1 < n_tiles) load_tile((t + 1) * BK);
    const unsigned long long t1 = stamp();
    const float* xb_ = &xs[buf][half * LDX + l32];
    const float* wb_ = &ws[buf][half * LDW + wave * 32 + l32];
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xb_[kk * LDX], wb_[kk * LDW], acc, 0, 0, 0);
    const unsigned long long t2 = stamp();
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) alone (gfx9 encoding: vmcnt in bits 3:0 and 15:14)
    const unsigned long long t3 = stamp();
    if (t + 1 < n_tiles) store_tile(buf ^ 1);
    const unsigned long long t4 = stamp();
    __syncthreads();
    const unsigned long long t5 = stamp();
    sum[0] += t1 - t0b; sum[1] += t2 - t1; sum[2] += t3 - t2; sum[3] += t4 - t3; sum[4] += t5 - t4;
    sum[5] += t0b - t0;
  }
  if (lane == 0) {
    unsigned long long* d = stamps + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * WM + wave) * 6;
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = sum[i];
  }
  const int m = m0 + wave * 32 + l32;
  if (m >= M) return;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int col = n0 + 8 * g + 4 * half;
    if (col >= n_total) continue;
    const int b = col / HW;
    *reinterpret_cast<float4*>(y + ((long long)b * M + m) * HW + (col - b * HW)) =
        make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
  }
}

#define CK(e)                                                                 \
  do {                                                                        \
    hipError_t e_ = (e);                                                      \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(e_));                 \
      exit(1);                                                                \
    }                                                                         \
  } while (0)

template <int WM, int BK>
static void run(int K, int M, int HW, int B) {
  const int n_total = B * HW, BM = 32 * WM;
  const dim3 grid((n_total + 31) / 32, (M + BM - 1) / BM), block(64 * WM);
  const size_t nx = (size_t)B * K * HW, nw = (size_t)M * K, ny = (size_t)B * M * HW, ng = (size_t)B * K;
  const size_t ns = (size_t)grid.x * grid.y * WM * 6;
  std::vector<float> h(nx > nw ? nx : nw);
  for (size_t i = 0; i < h.size(); ++i) h[i] = (float)((i * 2654435761u >> 8) & 1023) / 1024.0f - 0.5f;
  float *x, *w, *g, *y;
  unsigned long long* s;
  CK(hipMalloc(&x, nx * 4)); CK(hipMalloc(&w, nw * 4)); CK(hipMalloc(&g, ng * 4)); CK(hipMalloc(&y, ny * 4));
  CK(hipMalloc(&s, ns * 8));
  CK(hipMemcpy(x, h.data(), nx * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(w, h.data(), nw * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(g, h.data(), ng * 4, hipMemcpyHostToDevice));
  for (int rep = 0; rep < 3; ++rep)  // the last run's stamps are read: caches and clocks as in a steady loop
    hipLaunchKernelGGL((k13_tall_stamped<WM, BK>), grid, block, 0, 0, x, w, g, y, M, K, HW, n_total, s);
  CK(hipDeviceSynchronize());
  std::vector<unsigned long long> hs(ns);
  CK(hipMemcpy(hs.data(), s, ns * 8, hipMemcpyDeviceToHost));
  double tot[6] = {0, 0, 0, 0, 0, 0};
  for (size_t i = 0; i < ns; ++i) tot[i % 6] += (double)hs[i];
  const double waves = (double)ns / 6, tiles = (K + BK - 1) / BK;
  const double own = tot[5] / waves / tiles;
  double seg[5], all = 0;
  for (int i = 0; i < 5; ++i) { seg[i] = tot[i] / waves / tiles - own; if (seg[i] < 0) seg[i] = 0; all += seg[i]; }
  printf("| %d -> %d, HW %d, B %d | tall<%d, BK %d>, %u x %u workgroups | %.0f | %.1f %% | %.1f %% | %.1f %% | %.1f %% | %.1f %% | %.0f |\n",
         K, M, HW, B, WM, BK, grid.x, grid.y, all, 100 * seg[0] / all, 100 * seg[1] / all, 100 * seg[2] / all,
         100 * seg[3] / all, 100 * seg[4] / all, own);
  CK(hipFree(x)); CK(hipFree(w)); CK(hipFree(g)); CK(hipFree(y)); CK(hipFree(s));
}

int main() {
  printf("| shape | configuration | clock ticks per k-tile (s_memtime, stamps subtracted) | issue loads | LDS reads + MFMA | wait for global loads | gate + LDS writes | barrier | one stamp |\n");
  printf("|---|---|---|---|---|---|---|---|---|\n");
  run<4, 32>(1536, 256, 64, 64);
  run<5, 16>(960, 160, 256, 64);
  return 0;
}
