// Sustained rate of the block-scaled MFMA under the chip's power limit (gfx950), beside the bf16 form the GEMMs use today.
// A pure stream of v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, random operands and random E8M0 scales near 2^0) against
// v_mfma_f32_16x16x32_bf16 (random bf16 in [-1, 1)): 8 waves per CU, 8 independent accumulators per wave, ~1.5 s of
// back-to-back launches on every CU.  Reports TFLOP/s and the shader clock (s_memtime over s_memrealtime, 100 MHz).
// This bounds what an MXFP8 GEMM can gain (MXFP8 section; profiles/r07_mxfp8_probe.txt).
//   build: hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/mxfp8_probe.hip -o tools/build/mxfp8_probe
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

#define CHECK(x)                                                                              \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) {                                                                   \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));       \
      exit(1);                                                                                \
    }                                                                                         \
  } while (0)

struct Clocks { unsigned long long shader0, real0, shader1, real1; };

template <bool MX>
__global__ __launch_bounds__(512, 2) void stream_kernel(const int* __restrict__ src, float* __restrict__ out, int iters,
                                                        Clocks* clk) {
  if (blockIdx.x == 0 && threadIdx.x == 0) { clk->shader0 = __builtin_amdgcn_s_memtime(); clk->real0 = __builtin_amdgcn_s_memrealtime(); }
  const int lane = threadIdx.x & 63;
  const int* s = src + ((blockIdx.x * 8 + (threadIdx.x >> 6)) & 255) * 64 * 10 + lane * 10;
  i32x8_t a = {s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
  i32x8_t b = {s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8]};
  const int sa = s[9] & 0xff, sb = (s[9] >> 8) & 0xff;
  f32x4_t acc[8];
  for (int i = 0; i < 8; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if constexpr (MX)
        acc[i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc[i], 0, 0, 0, sa, 0, sb);
      else
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, __builtin_shufflevector(a, a, 0, 1, 2, 3)),
                                                         __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(b, b, 0, 1, 2, 3)),
                                                         acc[i], 0, 0, 0);
    }
  }
  float r = 0.f;
  for (int i = 0; i < 8; ++i) r += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
  if (blockIdx.x == 0 && threadIdx.x == 0) { clk->shader1 = __builtin_amdgcn_s_memtime(); clk->real1 = __builtin_amdgcn_s_memrealtime(); }
}

static uint32_t rng = 12345u;
static uint32_t next() { rng = rng * 1664525u + 1013904223u; return rng >> 8; }

int main(int argc, char** argv) {
  const double seconds = argc > 1 ? atof(argv[1]) : 1.5;
  int dev = 0, cus = 0;
  CHECK(hipGetDevice(&dev));
  CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  // 256 waves' worth of 64 lanes x 10 words: 8 operand words + 1 spare + one scale word
  std::vector<int> hs(256 * 64 * 10);
  for (size_t i = 0; i < hs.size(); ++i) {
    if (i % 10 == 9) { hs[i] = (int)((125u + next() % 5u) | ((125u + next() % 5u) << 8)); continue; }   // scales 2^-2 .. 2^2
    uint32_t w = 0;
    for (int j = 0; j < 4; ++j) {
      uint32_t byte = next() & 0xffu;
      if ((byte & 0x7fu) == 0x7fu) byte ^= 1u;   // no e4m3 NaN
      w |= byte << (8 * j);
    }
    hs[i] = (int)w;
  }
  std::vector<int> hb = hs;   // the bf16 probe: operand words are bf16 pairs in [-1, 1)
  for (size_t i = 0; i < hb.size(); ++i) {
    if (i % 10 == 9) continue;
    uint32_t w = 0;
    for (int h = 0; h < 2; ++h) {
      const float f = (float)(next() % 2000000) / 1000000.f - 1.f;
      uint32_t u; memcpy(&u, &f, 4);
      w |= (u >> 16) << (16 * h);
    }
    hb[i] = (int)w;
  }
  int *d_mx, *d_bf;
  float* d_out;
  Clocks* d_clk;
  const int blocks = cus;   // one 512-thread workgroup per CU = 8 waves / CU
  CHECK(hipMalloc(&d_mx, hs.size() * 4));
  CHECK(hipMalloc(&d_bf, hb.size() * 4));
  CHECK(hipMalloc(&d_out, (size_t)blocks * 512 * 4));
  CHECK(hipMalloc(&d_clk, sizeof(Clocks)));
  CHECK(hipMemcpy(d_mx, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_bf, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
  printf("# mxfp8_probe: %d CUs, %.1f s per probe, 8 waves/CU, 8 independent accumulators per wave, random operands\n", cus, seconds);
  for (int which = 0; which < 2; ++which) {
    const bool mx = which == 1;
    const int iters = 4096;
    const double flop_per_launch = (double)blocks * 8 * iters * 8 * (mx ? 2.0 * 16 * 16 * 128 : 2.0 * 16 * 16 * 32);
    auto launch = [&] {
      if (mx) hipLaunchKernelGGL(stream_kernel<true>, dim3(blocks), dim3(512), 0, 0, d_mx, d_out, iters, d_clk);
      else hipLaunchKernelGGL(stream_kernel<false>, dim3(blocks), dim3(512), 0, 0, d_bf, d_out, iters, d_clk);
    };
    for (int w = 0; w < 20; ++w) launch();
    CHECK(hipDeviceSynchronize());
    std::vector<double> rates, clocks;
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::duration<double>(seconds);
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    while (std::chrono::steady_clock::now() < t_end) {
      CHECK(hipEventRecord(e0, 0));
      for (int r = 0; r < 10; ++r) launch();
      CHECK(hipEventRecord(e1, 0));
      CHECK(hipEventSynchronize(e1));
      float ms = 0.f;
      CHECK(hipEventElapsedTime(&ms, e0, e1));
      Clocks c;
      CHECK(hipMemcpy(&c, d_clk, sizeof(c), hipMemcpyDeviceToHost));
      rates.push_back(10 * flop_per_launch / (ms * 1e-3) / 1e12);
      clocks.push_back((double)(c.shader1 - c.shader0) / ((double)(c.real1 - c.real0) / 100e6) / 1e9);
    }
    CHECK(hipGetLastError());
    const size_t n = rates.size(), h = n / 2;
    double r = 0, c = 0;
    for (size_t i = h; i < n; ++i) { r += rates[i]; c += clocks[i]; }
    r /= (double)(n - h);
    c /= (double)(n - h);
    const double peak = mx ? 5000.0 : 2500.0;
    printf("%-44s first %7.1f  steady %7.1f TF/s  (%.3f of %.0f)  clock %.3f GHz  [%zu samples]\n",
           mx ? "mfma_scale 16x16x128 f8f6f4 (e4m3 x e4m3)" : "mfma 16x16x32 bf16", rates[0], r, r / peak, peak, c, n);
  }
  return 0;
}
