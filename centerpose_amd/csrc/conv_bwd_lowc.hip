// The low-channel 3x3 path of cp_conv2d_backward_nhwc (conv_bwd.hip: cp_conv_backward_lowc): 3x3 / pad 1, stride 1 or 2,
// Cin == 16, Cout 16 or 32 -- dla_34's base.level0.0 (16 -> 16, stride 1) and base.level1.0 (16 -> 32, stride 2) of
// pose_dla_dcn.py:247-271, the two convolutions on the network's largest activations.  conv_bwd.hip's MFMA kernels need
// Cin % 32 == 0; its generic kernels walk tens of thousands of pixels per thread.  Exact float32 on v_mfma_f32_16x16x4_f32,
// every sum in an order fixed by the shape, no atomics.  Both kernels read gs [B,Ho,Wo,Cout]: grad_out in place, or
// stage_kernel's gated copy (CoP == Cout on this path); the bias gradient is stage_kernel's as on the other paths.
//
// Weight gradient (lowc_wgrad_kernel): D[co][tap * 16 + c] = sum over output pixels q of gs[q][co] * x[q * stride + tap - 1][c].
// M = Cout (one or two 16-row tiles), N = 144 = nine tap tiles of exactly one tap x 16 channels, K = output pixels, four per
// MFMA.  stem_bwd.hip's scheme:
//   * A workgroup is one slab and walks a contiguous run of output TILES.  Per tile it stages the x patch with its one-pixel
//     halo into LDS from whole 64-byte pixel rows (float4 per lane, a patch row is contiguous in memory); pixels outside the
//     image are zeros by select on a clamped address.
//   * Tile: 8 output rows x 64 columns at stride 1 (patch 10 x 66 pixels x 64 B = 42 240 B, three workgroups per CU of 160 KiB),
//     8 x 16 at stride 2 (patch 17 x 33 x 64 B = 35 904 B, four per CU).  At stride 2 the patch is about four times the tile,
//     so the tile is a quarter as wide: 8 x 64 would need 17 x 129 x 64 B = 140 KB, one workgroup per CU, and 8 x 32 (70 KB)
//     exactly two with nothing to spare, while the 33-pixel rows of 8 x 16 are still 2112 contiguous bytes.  The halo costs
//     29 % (stride 1) / 10 % (stride 2) more x reads than the tile holds, nearly all of them L2 hits on the neighbour's lines.
//   * A wave takes every fourth group of four neighbouring output pixels of a row.  A operand: gs in place, lane = (pixel of
//     the four, co): 64 contiguous bytes per pixel and co tile.  B operand: one LDS word per tap, lane = (pixel, c); the tap's
//     offset in the patch is a compile-time constant.  The A loads of four steps are issued before the chunk's first MFMA.
//     Pixels past the ragged edge: clamped address, zero by select.
//   * The four waves' accumulators are added in LDS in wave order and stored as the slab [Cout][144], k = tap * 16 + c: the
//     layout and the two_level_sum order of conv_bwd.hip's wgrad_reduce_kernel, which sums the slabs into grad_w.
//
// Data gradient (lowc_dgrad_kernel): grad_x[p][c] = sum over taps and co of gs[(p + 1 - tap) / stride][co] * w[co][c][tap].
// The MFMA is turned so that the STORE is whole lines: M = the 16 input channels, N = 16 neighbouring pixels of a row, K = co
// (four per MFMA), so D[c = 4 (lane >> 4) + e][pixel = lane & 15] is one float4 per lane and a wave instruction writes 16
// pixels x 64 B = 1024 contiguous bytes.  A[c][co] = w[co][c][tap] is held in registers (9 x Cout / 4 words per lane), read once
// per workgroup, which then walks a contiguous run of tiles.  B[co][pixel] comes from the gs tile staged with its halo in LDS
// (float4 global reads of whole pixel rows, zeros by select outside the image); a lane reads one float4 = four co of its pixel
// per four MFMAs (MFMA j takes co = 16 blk + 4 (lane >> 4) + j from both operands), and the pixel pitch is Cout + 4 words so
// that the 16 pixels of a read fall on distinct banks.
//   * Stride 1: tile 8 x 32 input pixels, gs patch 10 x 34 pixels; nine taps, patch pixel (ry + 2 - ky, cx + 2 - kx).
//   * Stride 2: dgrad_s2_kernel's sub-pixel form.  Tile 8 x 32 class coordinates (jy, jx) = 16 x 64 input pixels, gs patch
//     9 x 33.  Input pixel (2 jy + py, 2 jx + px) receives only the taps with ky = py + 1, kx = px + 1 (mod 2), from gs pixel
//     (jy + (py + 1 - ky) / 2, jx + (px + 1 - kx) / 2): 1, 2, 2 and 4 taps, no zero-inserted work.  A wave job is one (jy, py)
//     and 16 jx with BOTH px classes in two accumulators; the two are interleaved across lanes (two rounds of shuffles) so that
//     each store instruction again covers 16 neighbouring pixels = 1024 contiguous bytes of the interleaved NHWC grad_x.  Odd H
//     and W: the classes' unequal extents are a per-lane select of the store's execution (pixel inside the image), never a
//     branch around a class.
#include "op_common.h"
#include "igemm_common.h"

#include <algorithm>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int MAX_WG = 1024;  // workgroups (weight gradient: slabs) at most: four per CU
constexpr int WG_TR = 8;      // weight gradient: output rows of a tile
constexpr int DG_TY = 8, DG_TX = 32;  // data gradient: rows x columns of a tile (stride 2: of class coordinates)
constexpr int wg_tc(int stride) { return stride == 1 ? 64 : 16; }

ConvLowcPlan run_plan(int B, int ty, int tx) {
    ConvLowcPlan p;
    p.tiles_y = ty;
    p.tiles_x = tx;
    p.tiles = B * ty * tx;
    p.tiles_per_wg = (p.tiles + MAX_WG - 1) / MAX_WG;
    p.wgs = (p.tiles + p.tiles_per_wg - 1) / p.tiles_per_wg;
    return p;
}

template <int S, int NCO>
__global__ __launch_bounds__(256) void lowc_wgrad_kernel(const float* __restrict__ gs, const float* __restrict__ x,
                                                         float* __restrict__ slab, int H, int W, int Ho, int Wo, int tiles_y,
                                                         int tiles_x, int tiles, int tiles_per_wg) {
    constexpr int TR = WG_TR, TC = wg_tc(S), IR = (TR - 1) * S + 3, IC = (TC - 1) * S + 3, Cout = 16 * NCO, U = 4;
    constexpr int GPR = TC / 4, NG = TR * GPR;  // groups of four pixels: per row, per tile
    constexpr int PATCH = IR * IC * 16, SLAB = Cout * 144;
    static_assert(NG % (4 * U) == 0, "whole chunks per wave");
    __shared__ __attribute__((aligned(16))) float lds[PATCH > SLAB ? PATCH : SLAB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, kq = lane >> 4;
    f32x4 acc[NCO][9];
#pragma unroll
    for (int ct = 0; ct < NCO; ++ct)
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[ct][t] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int t_beg = blockIdx.x * tiles_per_wg, t_end = min(tiles, t_beg + tiles_per_wg);
    for (int t = t_beg; t < t_end; ++t) {
        const int b = t / (tiles_y * tiles_x), tr = t - b * tiles_y * tiles_x, ty = tr / tiles_x, tx = tr - ty * tiles_x;
        const int oy0 = ty * TR, ox0 = tx * TC, iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
        __syncthreads();  // the previous tile's patch has been read
        for (int idx = threadIdx.x; idx < IR * IC * 4; idx += 256) {
            const int rr = idx / (IC * 4), rem = idx - rr * IC * 4, cc = rem >> 2, q4 = rem & 3;
            const int iy = iy0 + rr, ix = ix0 + cc;
            const bool in = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
            const float4 v = ld4(x + (((size_t)b * H + (in ? iy : 0)) * W + (in ? ix : 0)) * 16 + 4 * q4);
            *reinterpret_cast<float4*>(lds + (rr * IC + cc) * 16 + 4 * q4) = in ? v : zero4();
        }
        __syncthreads();
        // group q = wave + 4 j: row q / GPR, columns 4 (q % GPR) + 0..3
        for (int j0 = 0; j0 < NG / 4; j0 += U) {
            float a[U][NCO];
            int poff[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int q = wave + 4 * (j0 + u), ry = q / GPR, cx = (q - ry * GPR) * 4 + kq;
                const int oy = oy0 + ry, ox = ox0 + cx;
                const bool ok = oy < Ho && ox < Wo;
                const size_t p = (((size_t)b * Ho + (ok ? oy : 0)) * Wo + (ok ? ox : 0)) * Cout + r;
                poff[u] = (ry * S * IC + cx * S) * 16 + r;
#pragma unroll
                for (int ct = 0; ct < NCO; ++ct) {
                    const float v = gs[p + 16 * ct];
                    a[u][ct] = ok ? v : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const float bv = lds[poff[u] + ((tap / 3) * IC + tap % 3) * 16];
#pragma unroll
                    for (int ct = 0; ct < NCO; ++ct) acc[ct][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][ct], bv, acc[ct][tap], 0, 0, 0);
                }
        }
    }
    // the four waves' accumulators, added in wave order: D[co = 16 ct + 4 (lane >> 4) + e][k = 16 tap + (lane & 15)]
    for (int w = 0; w < 4; ++w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int ct = 0; ct < NCO; ++ct)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int i = (ct * 16 + kq * 4 + e) * 144 + tap * 16 + r;
                        lds[i] = w ? lds[i] + acc[ct][tap][e] : acc[ct][tap][e];
                    }
        }
    }
    __syncthreads();
    float* out = slab + (size_t)blockIdx.x * SLAB;
    for (int i = threadIdx.x; i < SLAB; i += 256) out[i] = lds[i];
}

template <int S, int NB>
__global__ __launch_bounds__(256) void lowc_dgrad_kernel(const float* __restrict__ gs, const float* __restrict__ w,
                                                         float* __restrict__ gx, int H, int W, int Ho, int Wo, int tiles_y,
                                                         int tiles_x, int tiles, int tiles_per_wg) {
    constexpr int Cout = 16 * NB, PITCH = Cout + 4, C4 = Cout / 4;
    constexpr int PR = S == 1 ? DG_TY + 2 : DG_TY + 1, PC = S == 1 ? DG_TX + 2 : DG_TX + 1;
    __shared__ __attribute__((aligned(16))) float lds[PR * PC * PITCH];
    const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // A[c = r][co = 16 blk + 4 kq + j] of every tap
    float wr[9][NB][4];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int blk = 0; blk < NB; ++blk)
#pragma unroll
            for (int j = 0; j < 4; ++j) wr[tap][blk][j] = w[((16 * blk + 4 * kq + j) * 16 + r) * 9 + tap];

    const int t_beg = blockIdx.x * tiles_per_wg, t_end = min(tiles, t_beg + tiles_per_wg);
    for (int t = t_beg; t < t_end; ++t) {
        const int b = t / (tiles_y * tiles_x), tr = t - b * tiles_y * tiles_x, ty = tr / tiles_x, tx = tr - ty * tiles_x;
        const int y0 = ty * DG_TY, x0 = tx * DG_TX;            // stride 1: input pixels; stride 2: class coordinates
        const int oyb = S == 1 ? y0 - 1 : y0, oxb = S == 1 ? x0 - 1 : x0;  // the patch's first gs pixel
        __syncthreads();  // the previous tile's patch has been read
        for (int idx = threadIdx.x; idx < PR * PC * C4; idx += 256) {
            const int pr = idx / (PC * C4), rem = idx - pr * PC * C4, pc = rem / C4, q4 = rem - pc * C4;
            const int oy = oyb + pr, ox = oxb + pc;
            const bool in = (unsigned)oy < (unsigned)Ho && (unsigned)ox < (unsigned)Wo;
            const float4 v = ld4(gs + (((size_t)b * Ho + (in ? oy : 0)) * Wo + (in ? ox : 0)) * Cout + 4 * q4);
            *reinterpret_cast<float4*>(lds + (pr * PC + pc) * PITCH + 4 * q4) = in ? v : zero4();
        }
        __syncthreads();
        if constexpr (S == 1) {
            // job = (row, 16-pixel group): 16 per tile, four per wave
            for (int i = 0; i < DG_TY * (DG_TX / 16) / 4; ++i) {
                const int job = wave + 4 * i, ry = job >> 1, cx = (job & 1) * 16 + r;
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float* bp = lds + ((ry + 2 - ky) * PC + cx + 2 - kx) * PITCH + 4 * kq;
#pragma unroll
                        for (int blk = 0; blk < NB; ++blk) {
                            const float4 bv = *reinterpret_cast<const float4*>(bp + 16 * blk);
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[ky * 3 + kx][blk][0], bv.x, acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[ky * 3 + kx][blk][1], bv.y, acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[ky * 3 + kx][blk][2], bv.z, acc, 0, 0, 0);
                            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[ky * 3 + kx][blk][3], bv.w, acc, 0, 0, 0);
                        }
                    }
                const int iy = y0 + ry, ix = x0 + cx;
                if (iy < H && ix < W)
                    *reinterpret_cast<float4*>(gx + (((size_t)b * H + iy) * W + ix) * 16 + 4 * kq) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            }
        } else {
            // job = (class row jy, py, 16-jx group): 32 per tile, eight per wave; both px classes
            for (int i = 0; i < DG_TY * 2 * (DG_TX / 16) / 4; ++i) {
                const int job = wave + 4 * i, g = job & 1, py = (job >> 1) & 1, jyl = job >> 2, jxl = g * 16 + r;
                f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    if ((py + 1 - ky) & 1) continue;  // wave-uniform
                    const float* bp = lds + ((jyl + ((py + 1 - ky) >> 1)) * PC + jxl) * PITCH + 4 * kq;
#pragma unroll
                    for (int blk = 0; blk < NB; ++blk) {
                        const float4 b0 = *reinterpret_cast<const float4*>(bp + 16 * blk);          // gs pixel jx
                        const float4 b1 = *reinterpret_cast<const float4*>(bp + PITCH + 16 * blk);  // gs pixel jx + 1
                        const float v0[4] = {b0.x, b0.y, b0.z, b0.w}, v1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[ky * 3 + 1][blk][j], v0[j], acc0, 0, 0, 0);  // px 0: kx 1
                            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[ky * 3 + 0][blk][j], v1[j], acc1, 0, 0, 0);  // px 1: kx 0
                            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[ky * 3 + 2][blk][j], v0[j], acc1, 0, 0, 0);  //       kx 2
                        }
                    }
                }
                // store round h: lane (r, kq) writes input column 2 (8 h + r / 2) + (r & 1) of the group, channels 4 kq .. + 3:
                // class px = r & 1 of the lane that holds jx = 8 h + r / 2
                const int iy = 2 * (y0 + jyl) + py;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int src = kq * 16 + 8 * h + (r >> 1);
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float e0 = __shfl(acc0[e], src), e1 = __shfl(acc1[e], src);
                        v[e] = (r & 1) ? e1 : e0;
                    }
                    const int ix = 2 * (x0 + g * 16 + 8 * h) + r;
                    if (iy < H && ix < W)
                        *reinterpret_cast<float4*>(gx + (((size_t)b * H + iy) * W + ix) * 16 + 4 * kq) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
    }
}

}  // namespace

ConvLowcPlan cp_conv_lowc_wgrad_plan(int B, int Ho, int Wo, int stride) {
    const int tc = wg_tc(stride);
    return run_plan(B, (Ho + WG_TR - 1) / WG_TR, (Wo + tc - 1) / tc);
}

ConvLowcPlan cp_conv_lowc_dgrad_plan(int B, int H, int W, int stride) {
    const int hj = stride == 1 ? H : (H + 1) / 2, wj = stride == 1 ? W : (W + 1) / 2;
    return run_plan(B, (hj + DG_TY - 1) / DG_TY, (wj + DG_TX - 1) / DG_TX);
}

size_t cp_conv_lowc_slab_bytes(int B, int Ho, int Wo, int Cout, int stride) {
    return (size_t)std::min(cp_conv_lowc_wgrad_plan(B, Ho, Wo, stride).tiles, MAX_WG) * Cout * 144 * sizeof(float);
}

int cp_launch_conv_lowc_wgrad(hipStream_t s, const ConvBwdArgs& a, const float* gs, const ConvLowcPlan& P, float* slab) {
    const int Ho = (a.H - 1) / a.stride + 1, Wo = (a.W - 1) / a.stride + 1;
#define CP_LOWC_WGRAD(S, NCO)                                                                                                 \
    hipLaunchKernelGGL((lowc_wgrad_kernel<S, NCO>), dim3(P.wgs), dim3(256), 0, s, gs, a.x, slab, a.H, a.W, Ho, Wo, P.tiles_y, \
                       P.tiles_x, P.tiles, P.tiles_per_wg)
    if (a.stride == 1) {
        if (a.Cout == 16) CP_LOWC_WGRAD(1, 1);
        else CP_LOWC_WGRAD(1, 2);
    } else {
        if (a.Cout == 16) CP_LOWC_WGRAD(2, 1);
        else CP_LOWC_WGRAD(2, 2);
    }
#undef CP_LOWC_WGRAD
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_conv_lowc_dgrad(hipStream_t s, const ConvBwdArgs& a, const float* gs) {
    const int Ho = (a.H - 1) / a.stride + 1, Wo = (a.W - 1) / a.stride + 1;
    const ConvLowcPlan P = cp_conv_lowc_dgrad_plan(a.B, a.H, a.W, a.stride);
#define CP_LOWC_DGRAD(S, NB)                                                                                                 \
    hipLaunchKernelGGL((lowc_dgrad_kernel<S, NB>), dim3(P.wgs), dim3(256), 0, s, gs, a.w, a.gx, a.H, a.W, Ho, Wo, P.tiles_y, \
                       P.tiles_x, P.tiles, P.tiles_per_wg)
    if (a.stride == 1) {
        if (a.Cout == 16) CP_LOWC_DGRAD(1, 1);
        else CP_LOWC_DGRAD(1, 2);
    } else {
        if (a.Cout == 16) CP_LOWC_DGRAD(2, 1);
        else CP_LOWC_DGRAD(2, 2);
    }
#undef CP_LOWC_DGRAD
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
