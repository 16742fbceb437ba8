// avt_rtree_score.h (private) — scoreByFeature (RTree.cpp:52-68) with getDepth (:41-50), the reference's float32 sequence in
// one place: k_rtree_predict, k_rtree_predict_dist (avt_rtree.hip) and the trainer's kernels (avt_rtree_train.hip) all call it.
// Both files are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#define RT_BACKGROUND_DEPTH 20.f

// The offsets f = (u.x, u.y, v.x, v.y) divided by the pixel's depth `sample`, rounded half away from zero (std::round), cast
// to int32 and added to the pixel (c, r); a probe outside [lox, hix] x [loy, hiy] (inclusive) or on zero depth reads
// BACKGROUND_DEPTH; the score is zu - zv.  `d` holds pixel (ox, oy) at index 0 with row stride `stride`: inference passes
// the whole image (ox = oy = 0) bounded by the region of interest (predictBest) or by the image (predict); the trainer passes
// an image's crop bounded by the crop, which reads what the whole image bounded by the image reads.
__device__ __forceinline__ float rt_score_by_feature(const float* __restrict__ d, int stride, int ox, int oy, int lox, int loy, int hix, int hiy,
                                                     int c, int r, float sample, float4 f) {
    const int ux = (int)roundf(__fdiv_rn(f.x, sample)) + c, uy = (int)roundf(__fdiv_rn(f.y, sample)) + r;
    const int vx = (int)roundf(__fdiv_rn(f.z, sample)) + c, vy = (int)roundf(__fdiv_rn(f.w, sample)) + r;
    float zu = RT_BACKGROUND_DEPTH, zv = RT_BACKGROUND_DEPTH;
    if (!(ux < lox || uy < loy || ux > hix || uy > hiy)) { zu = d[(size_t)(uy - oy) * stride + (ux - ox)]; if (zu == 0.0f) zu = RT_BACKGROUND_DEPTH; }
    if (!(vx < lox || vy < loy || vx > hix || vy > hiy)) { zv = d[(size_t)(vy - oy) * stride + (vx - ox)]; if (zv == 0.0f) zv = RT_BACKGROUND_DEPTH; }
    return zu - zv;
}
