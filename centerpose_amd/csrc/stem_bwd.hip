// Weight and bias gradient of the image stems (cp_conv2d_stem_backward): Conv2d(Cin in 1..3, Cout, 7, stride 1 | 2, padding 3)
// on a caller-owned NCHW image, the layer the 4-channel NHWC operators refuse -- pose_dla_dcn.py:247-271 (base_layer,
// pre_img_layer, pre_hm_layer) and resnet_dcn.py's conv1.  There is no data gradient: the input is an image.
//
// A float32 contraction D[co][tap] = sum over output pixels of g[pixel][co] * patch[pixel][tap], g = grad_out gated by y > 0
// where y is given, tap = (c, ky, kx) in the weight's own order; M = Cout, N = 49 Cin (at most 147), K = B Ho Wo.  It runs on
// v_mfma_f32_16x16x4_f32, four pixels per step:
//   * A workgroup walks a contiguous run of TILES, 8 output rows x 64 output columns of one image, and is one slab.  (Tiles, not
//     bands of whole rows: the staged input is 14 x 70 or 21 x 133 values per plane whatever the image's width.)
//   * Per tile it stages the input patch with its 6-row / 6-column halo into LDS, per plane, from plane reads that are contiguous
//     along W; pixels outside the image are zeros by select, the address is clamped.
//   * A wave takes every fourth group of four neighbouring pixels of a row.  Its A operand is grad_out read in place (lane =
//     (pixel of the four, co): 64 contiguous bytes per pixel and co tile), its B operand one LDS word per tap tile (lane = (pixel,
//     tap): the tap's offset in the patch is a per-lane constant, the pixel's is added).  The loads of four steps are issued
//     before the first MFMA of the chunk; pixels past the image's edge are clamped addresses and zeros.
//   * Tap column 49 Cin reads a constant 1 instead of the patch, so D[co][49 Cin] is the bias gradient's partial sum.
//   * The four waves' accumulators are added in LDS in wave order and stored as the workgroup's slab [Cout][49 Cin + 1].
//   * Cout above 64 (the hourglass's 3 -> 128 stem, large_hourglass.py:210) is split into channel blocks of at most 64, the
//     grid's second dimension: a block reads grad_out and y with the layer's Cout as the pixel stride, stages the same patch
//     once more (cheap next to the reads of grad_out) and writes its own rows of the slab.  One 128-wide instantiation would
//     hold 320 accumulator registers.  Up to 64 channels there is one block, and the arithmetic is what it was.
// stem_reduce_kernel sums the slabs with op_common.h's two_level_sum into grad_w (PyTorch layout) and grad_bias.  No atomics:
// every sum has an order fixed by the shape, so the results are bitwise reproducible.
#include "op_common.h"

#include <algorithm>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int TR = 8, TCW = 64;      // output rows x columns of a tile
constexpr int MAX_WG = 512;          // slabs at most
constexpr int LDS_FLOATS = 64 * 148; // the larger of: the staged patch 3 x 21 x 133 + 1, the slab Cout x (49 Cin + 1)

struct StemPlan {
    int Ho, Wo, tiles_y, tiles_x, tiles, tiles_per_wg, slabs;
};
StemPlan stem_plan(int B, int H, int W, int stride) {
    StemPlan p;
    p.Ho = (H - 1) / stride + 1;
    p.Wo = (W - 1) / stride + 1;
    p.tiles_y = (p.Ho + TR - 1) / TR;
    p.tiles_x = (p.Wo + TCW - 1) / TCW;
    const long long t = (long long)B * p.tiles_y * p.tiles_x;
    p.tiles = (int)t;
    p.tiles_per_wg = (int)((t + MAX_WG - 1) / MAX_WG);
    p.slabs = (p.tiles + p.tiles_per_wg - 1) / p.tiles_per_wg;
    return p;
}

template <int CIN, int NCO>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ go,
                                                         const float* __restrict__ y, float* __restrict__ slab, int H, int W, int Ho,
                                                         int Wo, int stride, int tiles_y, int tiles_x, int tiles, int tiles_per_wg,
                                                         int CT, int co_base) {
    // Cout: this workgroup's block of output channels, co0 .. co0 + Cout of the layer's CT (the pixel stride of go and y)
    constexpr int NT = CIN * 49, NS = NT + 1, NTT = (NS + 15) / 16, Cout = NCO * 16, U = 4;
    const int co0 = co_base + blockIdx.y * Cout;
    __shared__ float lds[LDS_FLOATS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
    const int IR = (TR - 1) * stride + 7, IC = (TCW - 1) * stride + 7, LW = IC | 1, ONE = CIN * IR * LW;
    // per tap tile: this lane's tap as an offset into the staged patch, and whether the pixel's offset is added (a real tap) or
    // not (the ones column; the columns past it read lds[0] and are dropped at the store)
    int toff[NTT];
    bool tpix[NTT];
#pragma unroll
    for (int tt = 0; tt < NTT; ++tt) {
        const int n = tt * 16 + r;
        const int c = n / 49, rem = n - c * 49, ky = rem / 7, kx = rem - ky * 7;
        tpix[tt] = n < NT;
        toff[tt] = n < NT ? (c * IR + ky) * LW + kx : (n == NT ? ONE : 0);
    }
    f32x4 acc[NCO][NTT];
#pragma unroll
    for (int ct = 0; ct < NCO; ++ct)
#pragma unroll
        for (int tt = 0; tt < NTT; ++tt) acc[ct][tt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int t_beg = blockIdx.x * tiles_per_wg, t_end = min(tiles, t_beg + tiles_per_wg);
    for (int t = t_beg; t < t_end; ++t) {
        const int b = t / (tiles_y * tiles_x), tr = t - b * tiles_y * tiles_x, ty = tr / tiles_x, tx = tr - ty * tiles_x;
        const int oy0 = ty * TR, ox0 = tx * TCW, iy0 = oy0 * stride - 3, ix0 = ox0 * stride - 3;
        __syncthreads();  // the previous tile's patch has been read
        for (int idx = threadIdx.x; idx < CIN * IR * IC; idx += 256) {
            const int c = idx / (IR * IC), rem = idx - c * IR * IC, rr = rem / IC, cc = rem - rr * IC;
            const int iy = iy0 + rr, ix = ix0 + cc;
            const bool in = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
            const float v = x[(((size_t)b * CIN + c) * H + (in ? iy : 0)) * W + (in ? ix : 0)];
            lds[(c * IR + rr) * LW + cc] = in ? v : 0.f;
        }
        if (threadIdx.x == 0) lds[ONE] = 1.f;
        __syncthreads();
        // 8 rows x 16 groups of four pixels; group q = wave + 4 j
        for (int j0 = 0; j0 < TR * TCW / 16; j0 += U) {
            float a[U][NCO];
            int poff[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = wave + 4 * (j0 + u), ry = q >> 4, cx = ((q & 15) << 2) + kq;
                const int oy = oy0 + ry, ox = ox0 + cx;
                const bool ok = oy < Ho && ox < Wo;
                const size_t p = (((size_t)b * Ho + (ok ? oy : 0)) * Wo + (ok ? ox : 0)) * CT + co0 + r;
                poff[u] = ry * stride * LW + cx * stride;
#pragma unroll
                for (int ct = 0; ct < NCO; ++ct) {
                    float v = go[p + 16 * ct];
                    if (y) v = cp_relu_gate(v, y[p + 16 * ct]);
                    a[u][ct] = ok ? v : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int tt = 0; tt < NTT; ++tt) {
                    const float bv = lds[toff[tt] + (tpix[tt] ? poff[u] : 0)];
#pragma unroll
                    for (int ct = 0; ct < NCO; ++ct) acc[ct][tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][ct], bv, acc[ct][tt], 0, 0, 0);
                }
        }
    }
    // the four waves' accumulators, added in wave order: D[co = 16 ct + 4 (lane >> 4) + e][tap = 16 tt + (lane & 15)]
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int ct = 0; ct < NCO; ++ct)
#pragma unroll
                for (int tt = 0; tt < NTT; ++tt) {
                    const int n = tt * 16 + r;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = (ct * 16 + kq * 4 + e) * NS + n;
                        if (n < NS) lds[i] = w ? lds[i] + acc[ct][tt][e] : acc[ct][tt][e];
                    }
                }
        }
    }
    __syncthreads();
    float* out = slab + ((size_t)blockIdx.x * CT + co0) * NS;
    for (int i = threadIdx.x; i < Cout * NS; i += 256) out[i] = lds[i];
}

// grad_w[co][tap] and grad_bias[co] = the slabs' [co][NT + 1] entries (two_level_sum)
__global__ __launch_bounds__(256) void stem_reduce_kernel(const float* __restrict__ slab, float* __restrict__ gw, float* __restrict__ gb,
                                                          int nslab, int Cout, int NT) {
    __shared__ float red[256];
    const int NS = NT + 1, n = Cout * NS;
    for (int base = blockIdx.x * 32; base < n; base += gridDim.x * 32) {  // (uniform per workgroup)
        const int i = base + (threadIdx.x & 31);
        const float t = two_level_sum(red, i < n, nslab, 0.f, [&](float v, int s) { return v + slab[(size_t)s * n + i]; });
        if (threadIdx.x < 32 && i < n) {
            const int co = i / NS, k = i - co * NS;
            if (k < NT) gw[co * NT + k] = t;
            else if (gb) gb[co] = t;
        }
        __syncthreads();
    }
}

template <int CIN>
void launch_wgrad(hipStream_t s, const StemBwdArgs& a, const StemPlan& P, float* slab) {
    // channel blocks of at most 64 (NCO <= 4: the accumulators' register budget): the full blocks as the grid's second dimension,
    // then the ragged one.  Every block writes its own rows of the slabs, so the order of the launches does not matter.
    const int full = a.Cout / 64, rest = a.Cout % 64 / 16;
#define CP_STEM_LAUNCH(NCO, BLOCKS, BASE)                                                                                     \
    hipLaunchKernelGGL((stem_wgrad_kernel<CIN, NCO>), dim3(P.slabs, BLOCKS), dim3(256), 0, s, a.x, a.go, a.y, slab, a.H, a.W, \
                       P.Ho, P.Wo, a.stride, P.tiles_y, P.tiles_x, P.tiles, P.tiles_per_wg, a.Cout, BASE)
    if (full) CP_STEM_LAUNCH(4, full, 0);
    if (rest == 1) CP_STEM_LAUNCH(1, 1, full * 64);
    else if (rest == 2) CP_STEM_LAUNCH(2, 1, full * 64);
    else if (rest == 3) CP_STEM_LAUNCH(3, 1, full * 64);
#undef CP_STEM_LAUNCH
}

}  // namespace

const char* cp_stem_backward_shape_error(int B, int H, int W, int Cin, int Cout, int stride, bool wide) {
    if (B < 1 || H < 1 || W < 1) return "conv2d_stem_backward: B, H and W must be at least 1";
    if (Cin < 1 || Cin > 3) return "conv2d_stem_backward: Cin must be 1, 2 or 3 (wider inputs take cp_conv2d_backward_nhwc)";
    if (wide && (Cout < 16 || Cout > 128 || Cout % 16)) return "conv2d_stem_backward: Cout must be a multiple of 16 from 16 to 128";
    if (!wide && (Cout < 16 || Cout > 64 || Cout % 16)) return "conv2d_stem_backward: Cout must be 16, 32, 48 or 64";
    if (stride != 1 && stride != 2) return "conv2d_stem_backward: stride must be 1 or 2";
    const long long ho = (H - 1) / stride + 1, wo = (W - 1) / stride + 1, lim = 0x7fffffffLL;
    if ((long long)B * Cin * H * W >= lim || (long long)B * ho * wo * Cout >= lim)
        return "conv2d_stem_backward: a tensor has 2^31 elements or more";
    return nullptr;
}

size_t cp_stem_backward_ws_bytes(int B, int H, int W, int Cin, int Cout, int stride) {
    Carve c{nullptr};
    c.take<float>((size_t)stem_plan(B, H, W, stride).slabs * Cout * (49 * Cin + 1) * sizeof(float));
    return c.off;
}

int cp_launch_stem_backward(hipStream_t s, const StemBwdArgs& a, void* ws) {
    const StemPlan P = stem_plan(a.B, a.H, a.W, a.stride);
    Carve c{(char*)ws};
    float* slab = c.take<float>((size_t)P.slabs * a.Cout * (49 * a.Cin + 1) * sizeof(float));
    if (a.Cin == 1) launch_wgrad<1>(s, a, P, slab);
    else if (a.Cin == 2) launch_wgrad<2>(s, a, P, slab);
    else launch_wgrad<3>(s, a, P, slab);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    const int n = a.Cout * (49 * a.Cin + 1);
    hipLaunchKernelGGL(stem_reduce_kernel, dim3((n + 31) / 32), dim3(256), 0, s, slab, a.gw, a.gb, P.slabs, a.Cout, 49 * a.Cin);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
