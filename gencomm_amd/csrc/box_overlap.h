// One entry of bbox_overlaps (opencood/utils/box_overlaps.pyx:17-57), shared by the overlap-matrix kernel of detect_kernels.h
// and the target assignment of target_kernels.h.  Precision follows the C Cython emits -- float differences, `+ 1.0` and the
// area products in double, float variables for box_area / iw / ih / ua, float product and division at the end.
#pragma once
#include "common.h"

namespace gc {

#pragma clang fp contract(off)

// the query box's area, a float variable of the outer loop in the source
__device__ __forceinline__ float bbox_query_area(float q0, float q1, float q2, float q3) {
  return (float)(((double)(q2 - q0) + 1.0) * ((double)(q3 - q1) + 1.0));
}

// overlap of box (b0, b1, b2, b3) with query box (q0, q1, q2, q3) of area `box_area` (bbox_query_area)
__device__ __forceinline__ float bbox_overlap_one(float b0, float b1, float b2, float b3, float q0, float q1, float q2, float q3,
                                                  float box_area) {
  float r = 0.f;
  const float iw = (float)((double)(fminf(b2, q2) - fmaxf(b0, q0)) + 1.0);
  if (iw > 0) {
    const float ih = (float)((double)(fminf(b3, q3) - fmaxf(b1, q1)) + 1.0);
    if (ih > 0) {
      const float ua = (float)(((double)(b2 - b0) + 1.0) * ((double)(b3 - b1) + 1.0) + (double)box_area - (double)(iw * ih));
      r = iw * ih / ua;
    }
  }
  return r;
}

#pragma clang fp contract(fast)

}  // namespace gc
