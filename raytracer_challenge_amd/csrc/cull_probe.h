// cull_probe.h — TEST INFRASTRUCTURE (include/rtc.h rtc_cull_probe_raw): one culling predicate of rtc_device.hpp on one caller-supplied
// record.  Included after rtc_device.hpp by the probe kernel (rtc_probe.hip) and by the CPU emulator's host loop, so both evaluate the
// functions the ray kernels inline and nothing else.  Doubles per record: RTC_CULL_* in rtc.h.
#pragma once

constexpr int cull_probe_doubles(int kind) {  // doubles per record; 0: no such kind
  return kind == 0 ? 18 : kind == 1 ? 17 : kind == 2 ? 12 : kind == 3 ? 3 : kind == 4 ? 9 : 0;
}

__device__ __forceinline__ unsigned char cull_probe_eval(int kind, const double* __restrict__ q) {
  if (kind == 0) {  // slab: fr[4], o[3], d[3], tlo, thi, lo[3], hi[3]
    const Ray o{q[4], q[5], q[6], q[7], q[8], q[9]};
    Frame32 F;
    make_frame(q, o, F);
    Trav T;
    T.tlo = q[10]; T.thi = q[11];
    float lo, hi, tn;
    t_interval32(T, lo, hi);
    return slab32c((float)q[12], (float)q[13], (float)q[14], (float)q[15], (float)q[16], (float)q[17], F, lo, hi, tn) ? 1 : 0;
  }
  if (kind == 1) {  // point: fr[4], o[3], d[3], t_hit, lo[3], hi[3]
    const Ray o{q[4], q[5], q[6], q[7], q[8], q[9]};
    Frame32 F;
    make_frame_point(q, o, q[10], F);
    return point_in_box((float)q[11], (float)q[12], (float)q[13], (float)q[14], (float)q[15], (float)q[16], F) ? 1 : 0;
  }
  if (kind == 2) {  // gate: lo[3], hi[3], o[3], d[3]
    const Ray r{q[6], q[7], q[8], q[9], q[10], q[11]};
    return group_box_hit(q, r) ? 1 : 0;
  }
  if (kind == 3) {  // plane: oy, dy, mode.  As at both call sites, which return on the reference's own |dy| < EPSILON rule first
    Trav T;        // (alone, plane_behind calls oy > 0, dy = -0 "behind": t = +inf)
    T.mode = (int)q[2];
    if (fabs(q[1] - 0.0) < EPS) return 0;
    return plane_behind(T, q[0], q[1]) ? 1 : 0;
  }
  if (kind == 4) {  // behind: point[3], light[3], unit normal[3]; backface_skip = 1
    DScene S;
    S.backface_skip = 1;
    return light_is_behind(S, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8]) ? 1 : 0;
  }
  return 0;
}
