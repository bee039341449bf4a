// rtc_bump.hip — the small kernel normal perturbation (include/rtc.h rtc_bump) adds to the device, hand-written HIP for gfx950: the one
// behind rtc_bump_normals, and its launcher, which rtc_scene.cpp calls.  (wf_shade's NP builds: rtc_kernels.hip; the one-kernel path's
// NP builds: rtc_feat.hip, RtcExt.)  Scenes without a bump record launch nothing of this file.
#include "rtc_device.hpp"

// The rule alone (rtc.h rtc_bump_normals): out[i] = the shading normal (steps 1-4) of a hit at points[i] on primitive prims[i] whose
// geometric normal is normals[i]; a primitive whose material has no record gets its normal back.
// One lane per item, grid-stride.  The inputs and the output are SoA (three rows of n doubles each; the host entry transposes), so a
// wave reads and writes whole lines; the primitive, its matrix and its record are gathers, 16 + 96 + 24 bytes per lane.
__global__ void __launch_bounds__(256) rtc_bump_normals_kernel(DScene S, DBumpTable bt, const int32_t* __restrict__ prims, const double* __restrict__ points,
                                                               const double* __restrict__ normals, unsigned long long n, double* __restrict__ out) {
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * blockDim.x) {
    const double nn[3] = {normals[i], normals[n + i], normals[2 * n + i]};
    double o[3] = {nn[0], nn[1], nn[2]};
    const int32_t prim = prims[i];
    if (prim >= 0 && prim < S.n_prims) {  // (the host entry refuses anything else; a lane never reads outside the tables)
      const DPrim P = S.prims[prim];
      const int32_t b = bt.mat_bump[P.mat];
      if (b >= 0) {
        const DBump B = bt.recs[b];
        rtc_bump_normal_at(B.kind, B.octaves, B.amplitude, B.frequency, S.xf_matinv + 16 * P.xform, points[i], points[n + i], points[2 * n + i], nn, o);
      }
    }
    out[i] = o[0]; out[n + i] = o[1]; out[2 * n + i] = o[2];
  }
}
void rtc_launch_bump_normals(const DScene& S, const DBumpTable& bt, const int32_t* prims, const double* points, const double* normals, unsigned long long n, double* out,
                             hipStream_t stream) {
  if (n == 0) return;
  const dim3 grid((unsigned)std::min<unsigned long long>((n + 255ull) / 256ull, 8192ull)), block(256);
  hipLaunchKernelGGL(rtc_bump_normals_kernel, grid, block, 0, stream, S, bt, prims, points, normals, n, out);
}
