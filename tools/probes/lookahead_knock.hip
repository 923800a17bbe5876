// Knock-out timing of k_lookahead (thor_amd/csrc/lookahead.hip): the library's kernel in a
// stand-alone harness, built once per -DLA_KNOCK=<mask> (0 whole, 1 no source loads, 2 no 256-candidate pass of
// the search, 4 no butterflies across lanes; the results of a knocked-out build are wrong, only the time is read).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I thor_amd/csrc -DLA_KNOCK=2 \
//         -o out/la_knock_2 tools/probes/lookahead_knock.hip
//   out/la_knock_2 [pairs = 16] [width = 3840] [height = 2160]
// Prints the median, minimum and maximum of 7 repetitions of 10 back-to-back calls, ms per call.
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "common.h"

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      fprintf(stderr, "%s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
      return THOR_ERR_HIP;                                                                 \
    }                                                                                      \
  } while (0)
// (quality.hip's, which the library's unity build has in front of lookahead.hip)
typedef const __attribute__((address_space(1))) uint8_t *sse_gptr;
typedef uint32_t __attribute__((aligned(1))) sse_u32u;
__device__ __forceinline__ uint32_t sse_ld4(sse_gptr p) { return *(const __attribute__((address_space(1))) sse_u32u *)p; }

#include "lookahead.hip"

static int run(int n, int W, int H) {
  const size_t fs = (size_t)W * H;
  int bw = 0, bh = 0;
  if (thor_lookahead_blocks(W, H, &bw, &bh) < 0) return THOR_ERR_ARG;
  uint8_t *cur = nullptr, *ref = nullptr;
  thor_la_block_t *recs = nullptr;
  uint64_t *sums = nullptr;
  HIPCHK(hipMalloc(&cur, n * fs));
  HIPCHK(hipMalloc(&ref, n * fs));
  HIPCHK(hipMalloc(&recs, (size_t)n * bw * bh * sizeof(thor_la_block_t)));
  HIPCHK(hipMalloc(&sums, (size_t)n * 4 * sizeof(uint64_t)));
  std::vector<uint8_t> host(fs);
  uint32_t s = 12345;
  for (size_t i = 0; i < fs; i++) host[i] = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
  for (int i = 0; i < n; i++) {  // every frame the same noise, the reference two rows and some bytes further on
    HIPCHK(hipMemcpy(cur + i * fs, host.data(), fs, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ref + i * fs, host.data() + 2 * W + 6, fs - 2 * W - 6, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ref + i * fs + fs - 2 * W - 6, host.data(), 2 * W + 6, hipMemcpyHostToDevice));
  }
  std::vector<thor_yuv_planes_t> pc(n), pr(n);
  for (int i = 0; i < n; i++) {
    pc[i] = thor_yuv_planes_t{cur + i * fs, nullptr, nullptr, W, W / 2};
    pr[i] = thor_yuv_planes_t{ref + i * fs, nullptr, nullptr, W, W / 2};
  }
  hipEvent_t a, b;
  HIPCHK(hipEventCreate(&a));
  HIPCHK(hipEventCreate(&b));
  for (int k = 0; k < 2; k++)
    if (thor_lookahead_i420(pc.data(), pr.data(), n, W, H, recs, sums, nullptr) != THOR_OK) return THOR_ERR_HIP;
  HIPCHK(hipDeviceSynchronize());
  std::vector<float> ms;
  for (int rep = 0; rep < 7; rep++) {
    HIPCHK(hipEventRecord(a, nullptr));
    for (int k = 0; k < 10; k++)
      if (thor_lookahead_i420(pc.data(), pr.data(), n, W, H, recs, sums, nullptr) != THOR_OK) return THOR_ERR_HIP;
    HIPCHK(hipEventRecord(b, nullptr));
    HIPCHK(hipEventSynchronize(b));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, a, b));
    ms.push_back(t / 10);
  }
  std::sort(ms.begin(), ms.end());
  uint64_t first[4];
  HIPCHK(hipMemcpy(first, sums, sizeof(first), hipMemcpyDeviceToHost));
  printf("LA_KNOCK=%d pairs=%d %dx%d ms_per_call median=%.4f min=%.4f max=%.4f (sums[0]: %llu %llu %llu %llu)\n", LA_KNOCK, n,
         W, H, ms[3], ms[0], ms[6], (unsigned long long)first[0], (unsigned long long)first[1], (unsigned long long)first[2],
         (unsigned long long)first[3]);
  (void)hipFree(cur), (void)hipFree(ref), (void)hipFree(recs), (void)hipFree(sums);
  return THOR_OK;
}

int main(int argc, char **argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 16, W = argc > 2 ? atoi(argv[2]) : 3840, H = argc > 3 ? atoi(argv[3]) : 2160;
  return run(n, W, H) == THOR_OK ? 0 : 1;
}
