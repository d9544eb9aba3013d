// Objectron box metrics on the device, float64: 3D IoU of oriented boxes, and evaluate_3d / evaluate_2d's symmetry
// sweeps with ADD, ADD-S and viewpoint error (the reference's src/tools/objectron_eval/eval_image_official.py:673-994
// over objectron/dataset/{box,iou}.py).  The numerics are box3d_common.h, shared with the host build the CPU tests pin
// to the reference's own output; this file only lays the work out.
//
// The work is independent (prediction, ground truth, rotation) triples of a few thousand dependent float64 operations
// each (Sutherland-Hodgman over 12 faces x 6 planes dominates): latency-bound, no MFMA, no packed math.
//   box_iou_kernel   one thread per (A, B) pair
//   box_eval_kernel  one workgroup of 128 lanes per matched pair, lane r takes rotation indices r, r + 128, ...; lane
//                    bests are combined by a tree reduction with the reference's sequential tie rule (first index)
// A clipped polygon is a runtime-sized list (up to MAXV = 10 vertices), so each lane keeps its two ping-pong polygon
// buffers in LDS rather than in a runtime-indexed private array (which would live in scratch memory): coordinate c of
// vertex k of lane l's buffer is at buf[(k * 3 + c) * LANES + l], consecutive lanes on consecutive doubles.
// Built for gfx950: box_eval_kernel 256 VGPRs, 560 B/lane private segment (the rotated 9 x 3 box, the pivoted 4 x 4
// solves and loops over vertices the compiler keeps runtime-indexed), 76.5 KB LDS per workgroup (two workgroups per
// CU); box_iou_kernel 244 VGPRs, 64 B/lane, 30 KB.  4096 pairs x 100 rotations: 1.19-1.27 ms of box_eval_kernel time
// on the MI355X (kernel trace, two builds), against 0.19 s per pair for the reference's CPU evaluator.
#include <cmath>

#include "cp_common.h"
#include "box3d_common.h"

namespace {

using namespace box3d;

constexpr int IOU_LANES = 64;
constexpr int EVAL_LANES = 128;

__global__ __launch_bounds__(IOU_LANES) void box_iou_kernel(const double* __restrict__ a, const double* __restrict__ b,
                                                           int n, double* __restrict__ iou) {
    __shared__ double poly[2][MAXV * 3 * IOU_LANES];
    const int lane = threadIdx.x;
    const int i = blockIdx.x * IOU_LANES + lane;
    if (i >= n) return;
    double va[27], vb[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) va[k] = a[(size_t)i * 27 + k], vb[k] = b[(size_t)i * 27 + k];
    int flags = 0;
    iou[i] = box_iou(va, vb, &poly[0][lane], &poly[1][lane], IOU_LANES, flags);
}

__global__ __launch_bounds__(EVAL_LANES) void box_eval_kernel(const double* __restrict__ pred3d,
                                                             const double* __restrict__ gt3d,
                                                             const double* __restrict__ pred2d,
                                                             const double* __restrict__ mo2c,
                                                             const double* __restrict__ proj,
                                                             const int* __restrict__ single, int num_symmetry,
                                                             double* __restrict__ out) {
    __shared__ double poly[2][MAXV * 3 * EVAL_LANES];
    __shared__ Best3 r3[EVAL_LANES];
    __shared__ Best2 r2[EVAL_LANES];
    __shared__ int rflags[EVAL_LANES];
    const int p = blockIdx.x, lane = threadIdx.x;
    double pr[27], gt[27], p2[18], M[16], P[16], Mi[16];
#pragma unroll
    for (int k = 0; k < 27; ++k) pr[k] = pred3d[(size_t)p * 27 + k], gt[k] = gt3d[(size_t)p * 27 + k];
#pragma unroll
    for (int k = 0; k < 18; ++k) p2[k] = pred2d[(size_t)p * 18 + k];
#pragma unroll
    for (int k = 0; k < 16; ++k) M[k] = mo2c[(size_t)p * 16 + k], P[k] = proj[(size_t)p * 16 + k];
    const bool ok = inv4(M, Mi);
    const int nr = single[p] ? 1 : num_symmetry;  // the mug break: index 0 of both sweeps only
    Best3 b3 = {0., 0., 0., 0., 0., -1, 0};
    Best2 b2 = {0., -1};
    int clip = 0;
    for (int r = lane; r < nr; r += EVAL_LANES) {
        eval_rotation3(pr, gt, r, num_symmetry, &poly[0][lane], &poly[1][lane], EVAL_LANES, b3, clip);
        if (ok) eval_rotation2(p2, gt, P, M, Mi, r, num_symmetry, b2);
    }
    r3[lane] = b3;
    r2[lane] = b2;
    rflags[lane] = clip;
    __syncthreads();
    for (int w = EVAL_LANES / 2; w > 0; w >>= 1) {
        if (lane < w) {
            if (better3(r3[lane + w], r3[lane])) r3[lane] = r3[lane + w];
            if (better2(r2[lane + w], r2[lane])) r2[lane] = r2[lane + w];
            rflags[lane] |= rflags[lane + w];
        }
        __syncthreads();
    }
    if (lane == 0) write_record(pr, gt, num_symmetry, r3[0], r2[0], rflags[0], ok, out + (size_t)p * CP_BOX_EVAL_STRIDE);
}

}  // namespace

int cp_launch_box_iou(hipStream_t s, const double* a, const double* b, int n, double* iou) {
    hipLaunchKernelGGL(box_iou_kernel, dim3((n + IOU_LANES - 1) / IOU_LANES), dim3(IOU_LANES), 0, s, a, b, n, iou);
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_box_eval(hipStream_t s, const double* pred3d, const double* gt3d, const double* pred2d, const double* mo2c,
                       const double* proj, const int* single, int n, int num_symmetry, double* out) {
    hipLaunchKernelGGL(box_eval_kernel, dim3(n), dim3(EVAL_LANES), 0, s, pred3d, gt3d, pred2d, mo2c, proj, single,
                       num_symmetry, out);
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}
