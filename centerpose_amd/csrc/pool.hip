// MaxPool2d for training (cp_maxpool2d_forward_nhwc / cp_maxpool2d_backward_nhwc): the two geometries of the reference's
// backbones on float32 NHWC tensors -- (kernel 2, stride 2, padding 0), Tree.downsample of pose_dla_dcn.py:211-224, which floors
// (an odd last row / column belongs to no window), and (3, 2, 1), resnet_dcn.py's maxpool, whose padding counts as -inf.
//
// Both directions use one definition of a window's winner, torch's: the taps inside the image are scanned in row-major order
// from (-inf, first tap) and a tap replaces the current winner only if it is strictly greater (or a NaN).  Ties are the normal
// case (the pooled tensors are ReLU outputs full of equal zeros), and the rule sends a tied window's gradient to its first tap.
//
// Forward: one thread per output pixel and float4 of channels.  Backward: a gather, one thread per grad_x pixel and float4 of
// channels; it finds the windows that cover its pixel (one at (2, 2, 0), up to four at (3, 2, 1)), recomputes each one's winner
// from x and adds that window's grad_out where the winner is its own pixel -- windows in (row, column) order, so the sum has a
// fixed order; no atomics and no saved index tensor.  Pixels no window covers get exact zeros.  Lanes read and write 16 bytes,
// and out-of-image taps are clamped addresses whose values a select drops, never a branch around the load.
#include "op_common.h"

#include <algorithm>

namespace {

constexpr int TPB = 256;

inline int grid_for(size_t n) { return (int)std::min<size_t>(std::max<size_t>((n + TPB - 1) / TPB, 1), 256 * 16); }

// The winner of the window at output pixel (oy, ox), per channel of the float4 at `c`: value in `best`, tap index (ky * K + kx)
// in `arg`
template <int K, int P>
__device__ __forceinline__ void window_winner(const float4* __restrict__ x4, size_t img, int H, int W, int C4, int c, int oy, int ox,
                                              float (&best)[4], int (&arg)[4]) {
    const int y0 = 2 * oy - P, x0 = 2 * ox - P;
    // the first tap inside the image (P <= 1: at most one row / column is cut off)
    const int first = (y0 < 0 ? 1 : 0) * K + (x0 < 0 ? 1 : 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        best[j] = -INFINITY;
        arg[j] = first;
    }
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const int y = y0 + ky, xx = x0 + kx;
            const bool in = (unsigned)y < (unsigned)H && (unsigned)xx < (unsigned)W;
            const float4 v4 = x4[img + ((size_t)(in ? y : 0) * W + (in ? xx : 0)) * C4 + c];
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool take = in && (v[j] > best[j] || v[j] != v[j]);
                best[j] = take ? v[j] : best[j];
                arg[j] = take ? ky * K + kx : arg[j];
            }
        }
}

template <int K, int P>
__global__ __launch_bounds__(TPB) void maxpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H, int W,
                                                          int C4, int Ho, int Wo) {
    const size_t total = (size_t)B * Ho * Wo * C4;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        size_t t = i / C4;
        const int ox = (int)(t % Wo);
        t /= Wo;
        const int oy = (int)(t % Ho);
        const size_t b = t / Ho;
        float best[4];
        int arg[4];
        window_winner<K, P>(x4, b * H * W * C4, H, W, C4, c, oy, ox, best, arg);
        reinterpret_cast<float4*>(out)[i] = make_float4(best[0], best[1], best[2], best[3]);
    }
}

template <int K, int P>
__global__ __launch_bounds__(TPB) void maxpool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ go,
                                                          float* __restrict__ gx, int B, int H, int W, int C4, int Ho, int Wo) {
    const size_t total = (size_t)B * H * W * C4;
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* go4 = reinterpret_cast<const float4*>(go);
    constexpr int NW = K == 2 ? 1 : 2;  // windows that can cover a pixel, per axis
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4);
        size_t t = i / C4;
        const int px = (int)(t % W);
        t /= W;
        const int py = (int)(t % H);
        const size_t b = t / H;
        float g[4] = {0.f, 0.f, 0.f, 0.f};
        // windows covering (py, px): 2 oy - P <= py <= 2 oy - P + K - 1.  (2, 2, 0): oy = py / 2.  (3, 2, 1): oy = py / 2 for an
        // even py (the centre tap), (py - 1) / 2 and (py + 1) / 2 for an odd one.
        const int oy0 = K == 2 ? py >> 1 : (py & 1 ? (py - 1) >> 1 : py >> 1);
        const int ox0 = K == 2 ? px >> 1 : (px & 1 ? (px - 1) >> 1 : px >> 1);
        const int ny = (K == 3 && (py & 1)) ? 2 : 1, nx = (K == 3 && (px & 1)) ? 2 : 1;
#pragma unroll
        for (int wy = 0; wy < NW; ++wy)
#pragma unroll
            for (int wx = 0; wx < NW; ++wx) {
                const int oy = oy0 + wy, ox = ox0 + wx;
                const bool live = wy < ny && wx < nx && oy < Ho && ox < Wo;
                const int oyc = live ? oy : 0, oxc = live ? ox : 0;  // (Ho, Wo >= 1)
                float best[4];
                int arg[4];
                window_winner<K, P>(x4, b * H * W * C4, H, W, C4, c, oyc, oxc, best, arg);
                const float4 d4 = go4[((b * Ho + oyc) * Wo + oxc) * C4 + c];
                const float d[4] = {d4.x, d4.y, d4.z, d4.w};
                const int mine = (py - (2 * oyc - P)) * K + (px - (2 * oxc - P));  // this pixel's tap index in that window
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = (live && arg[j] == mine) ? g[j] + d[j] : g[j];
            }
        reinterpret_cast<float4*>(gx)[i] = make_float4(g[0], g[1], g[2], g[3]);
    }
}

}  // namespace

bool cp_maxpool_geometry(int kernel, int stride, int pad) {
    return (kernel == 2 && stride == 2 && pad == 0) || (kernel == 3 && stride == 2 && pad == 1);
}

int cp_launch_maxpool_forward(hipStream_t s, const float* x, float* out, int B, int H, int W, int C, int kernel) {
    const int P = kernel == 2 ? 0 : 1, Ho = (H + 2 * P - kernel) / 2 + 1, Wo = (W + 2 * P - kernel) / 2 + 1;
    const int g = grid_for((size_t)B * Ho * Wo * (C / 4));
    if (kernel == 2) hipLaunchKernelGGL((maxpool_fwd_kernel<2, 0>), dim3(g), dim3(TPB), 0, s, x, out, B, H, W, C / 4, Ho, Wo);
    else hipLaunchKernelGGL((maxpool_fwd_kernel<3, 1>), dim3(g), dim3(TPB), 0, s, x, out, B, H, W, C / 4, Ho, Wo);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_maxpool_backward(hipStream_t s, const float* x, const float* go, float* gx, int B, int H, int W, int C, int kernel) {
    const int P = kernel == 2 ? 0 : 1, Ho = (H + 2 * P - kernel) / 2 + 1, Wo = (W + 2 * P - kernel) / 2 + 1;
    const int g = grid_for((size_t)B * H * W * (C / 4));
    if (kernel == 2) hipLaunchKernelGGL((maxpool_bwd_kernel<2, 0>), dim3(g), dim3(TPB), 0, s, x, go, gx, B, H, W, C / 4, Ho, Wo);
    else hipLaunchKernelGGL((maxpool_bwd_kernel<3, 1>), dim3(g), dim3(TPB), 0, s, x, go, gx, B, H, W, C / 4, Ho, Wo);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
