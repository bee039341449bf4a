// rtc_probe.hip — TEST INFRASTRUCTURE (include/rtc.h rtc_cull_probe_raw): the culling predicates of rtc_device.hpp, each alone, on the
// caller's records.  No scene table is read and no ray kernel launches anything of this file.
#include "rtc_device.hpp"
#include "cull_probe.h"

// One lane per record, grid-stride; a record is `stride` doubles, the answer one byte.
__global__ void __launch_bounds__(256) rtc_cull_probe_kernel(int kind, int stride, const double* __restrict__ records, unsigned long long n, unsigned char* __restrict__ out) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x)
    out[i] = cull_probe_eval(kind, records + i * (unsigned long long)stride);
}
int rtc_cull_probe_doubles(int kind) { return cull_probe_doubles(kind); }
void rtc_launch_cull_probe(int kind, const double* records, unsigned long long n, unsigned char* out, hipStream_t stream) {
  if (n == 0) return;
  const dim3 grid((unsigned)std::min<unsigned long long>((n + 255ull) / 256ull, 8192ull)), block(256);
  hipLaunchKernelGGL(rtc_cull_probe_kernel, grid, block, 0, stream, kind, cull_probe_doubles(kind), records, n, out);
}
