// Backward of the ordinary convolution (cp_conv2d_backward_nhwc): autograd's gradients of out = conv2d(x, w) + bias, dilation 1,
// groups 1, on the forward's layouts (x [B,H,W,Cin] NHWC, w [Cout,Cin,KH,KW], grad_out [B,Ho,Wo,Cout] NHWC).  It replaces
// torch.nn.Conv2d's backward in pose_dla_dcn.py:48-62 (BasicBlock), the Root / project 1x1s and DCNv2/dcn_v2.py:118-128
// (conv_offset_mask).  Float32 arithmetic by default; every sum has a fixed order; no atomics.  With CP_PREC_F16X3
// (cp_conv2d_backward_prec_nhwc) the two contractions of the MFMA path, steps 1 and 2, run on the split-binary16 kernels of
// conv_bwd16.hip; step 0, the slab reduction's order and the other two paths are the same in either mode.
//
// On the caller's stream:
//   0. stage    (stage_kernel) gs[q][CoP] = grad_out[q][co] * (y[q][co] > 0), zero in the pad lanes co >= Cout, CoP = Cout
//               rounded up to 32 on the MFMA path; the same pass leaves per-slab column sums, which bias_reduce_kernel adds in
//               a fixed order into grad_bias.  Skipped when there is nothing to gate, pad or sum (grad_out is then read in place).
//   1. wgrad    MFMA path: slab[s][co][k] = sum over the output rows of slab s of gs[q][co] * x[q * stride + tap - pad][c],
//               k = tap * Cin + c (wgrad_kernel: v_mfma_f32_32x32x2_f32 with K = output pixels, kernels 1x1 and 3x3, strides 1
//               and 2); wgrad_reduce_kernel sums the slabs in a fixed order into the PyTorch layout.  Generic path: one thread
//               per weight element and slab (wgrad_generic_kernel), the same reduction.
//   2. dgrad    stride 1, MFMA path: the exact-f32 implicit GEMM of igemm.hip on gs with the taps mirrored and the channel
//               roles swapped (pack_dgrad_kernel).  Stride 2, MFMA path: dgrad_s2_kernel, one dense contraction per input
//               pixel parity class (deconv16.hip's sub-pixel form), written straight into the interleaved grad_x.  Generic
//               path: a gather per grad_x element (dgrad_generic_kernel).  Not launched when the caller passes no grad_x.
// A third path takes the 16-channel 3x3s of DLA's levels 0-1 (cp_conv_backward_lowc: 3x3 / pad 1, stride 1 | 2, 16 -> 16 | 32,
// at least 4096 output pixels): steps 1 and 2 are conv_bwd_lowc.hip's kernels, step 0 and the slab reduction are the ones
// here.  cp_conv_backward_path names the path of a geometry, for the launch and for cp_conv2d_backward_path alike.
// The MFMA weight gradient and the stride-1 data gradient are also the library's only ones: cp_launch_conv_wgrad and
// cp_launch_conv_dgrad_pack / _s1 (cp_common.h) are what step 1 and 2 call, and what heads_bwd.hip calls for its 3x3 layer.
// cp_launch_rowsum_nchw, the NCHW bias gradient of dcn_bwd.hip and heads_bwd.hip, is here for the same reason.
#include "op_common.h"
#include "igemm_common.h"

#include <algorithm>

namespace {

// gs[q][c] (c < CoP) = gated grad_out, zero for c >= Cout, when `gs` is given; part[slab][c] = the slab's column sums when
// `part` is given.  A workgroup owns `slab_px` pixels (blockIdx.x) and CT channels (blockIdx.y; CT a power of two <= 64);
// thread = (pixel lane, channel), so a wave reads whole rows.  Sums: pixels ascending per pixel lane, then the pixel lanes in
// index order.
__global__ __launch_bounds__(256) void stage_kernel(const float* __restrict__ go, const float* __restrict__ y,
                                                    float* __restrict__ gs, float* __restrict__ part, int Q, int Cout, int CoP,
                                                    int CT, int slab_px) {
    __shared__ float red[256];
    const int PL = 256 / CT, cl = threadIdx.x % CT, pl = threadIdx.x / CT;
    const int q_beg = blockIdx.x * slab_px, q_end = min(Q, q_beg + slab_px);
    const int c = blockIdx.y * CT + cl;
    const bool cv = c < Cout, cw = gs && c < CoP;
    float sum = 0.f;
#pragma unroll 4
    for (int q = q_beg + pl; q < q_end; q += PL) {
        const size_t src = cv ? (size_t)q * Cout + c : 0;
        float v = go[src];
        if (y) v = cp_relu_gate(v, y[src]);
        v = cv ? v : 0.f;
        if (cw) gs[(size_t)q * CoP + c] = v;
        sum += v;
    }
    if (!part) return;
    red[threadIdx.x] = sum;
    __syncthreads();
    if (pl == 0 && c < CoP) {
        float t = red[cl];
        for (int j = 1; j < PL; ++j) t += red[j * CT + cl];
        part[(size_t)blockIdx.x * CoP + c] = t;
    }
}

// gb[c] = the slabs' partials (two_level_sum)
__global__ __launch_bounds__(256) void bias_reduce_kernel(const float* __restrict__ part, float* __restrict__ gb, int nslab, int Cout,
                                                          int CoP) {
    __shared__ float red[256];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31);
    const float t = two_level_sum(red, c < Cout, nslab, 0.f, [&](float v, int s) { return v + part[(size_t)s * CoP + c]; });
    if (threadIdx.x < 32 && c < Cout) gb[c] = t;
}

// slab[s][co][k] over the output rows [s * rows_per_slab, ...): D[co][k] with K = output pixels, two per MFMA step (lane half
// = pixel parity along x), eight steps' operands requested at a time.  A[co][q] = gs[q][h0 + lane & 31] (a 128-byte line per
// half), B[q][k] = x[q * stride + tap - pad][c0 + lane & 31] (likewise: a k tile of 32 stays inside one tap because
// Cin % 32 == 0); out-of-image taps and the ragged end of a row are zeros by select, never by a branch around the load.  A
// wave owns NH co tiles x 2 k tiles; the four waves of a workgroup take neighbouring k tile pairs of the same co tiles.
template <int NH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void wgrad_kernel(
    const float* __restrict__ gs, const float* __restrict__ x, float* __restrict__ slab, int rows, int Ho, int Wo, int H, int W,
    int Cin, int CoP, int KW, int taps, int stride, int pad, int rows_per_slab) {
    constexpr int WU = 8;
    const int TC = taps * Cin, KT = TC / 32, KJ = (KT + 1) / 2;
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int job = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int hg = job / KJ, kj = job - hg * KJ;
    if (hg * 32 * NH >= CoP) return;
    const int h0 = hg * 32 * NH;
    int dy[2], dx[2], c0[2];
    bool kv[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int kt = kj * 2 + n;
        kv[n] = kt < KT;
        const int k0 = kv[n] ? kt * 32 : 0, tap = k0 / Cin;
        c0[n] = k0 - tap * Cin;
        dy[n] = tap / KW - pad;
        dx[n] = tap - (tap / KW) * KW - pad;
    }
    f32x16 acc[NH][2];
#pragma unroll
    for (int t = 0; t < NH; ++t)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][n][e] = 0.f;
    const int row_beg = blockIdx.z * rows_per_slab, row_end = min(rows, row_beg + rows_per_slab);
    for (int row = row_beg; row < row_end; ++row) {
        const int b = row / Ho, oy = row - b * Ho;
        const float* arow = gs + (size_t)row * Wo * CoP + h0 + r;
        const float* brow[2];
        bool yv[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int iy = oy * stride + dy[n];
            yv[n] = kv[n] && (unsigned)iy < (unsigned)H;
            brow[n] = x + ((size_t)b * H + (yv[n] ? iy : 0)) * W * Cin + c0[n] + r;
        }
        // two pixels per step, WU steps per chunk: the chunk's operands are all requested before its first MFMA is issued, so
        // one memory round trip covers WU steps (steps past the row's end: clamped addresses, zeros)
        auto load = [&](int x0, float (&a)[NH], float (&bq)[2]) {
            const int ox = x0 + hh;
            const bool xv = ox < Wo;
            const int xc = xv ? ox : Wo - 1;
#pragma unroll
            for (int t = 0; t < NH; ++t) {
                const float v = arow[(size_t)xc * CoP + 32 * t];
                a[t] = xv ? v : 0.f;
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int ix = ox * stride + dx[n];
                const bool ok = xv && yv[n] && (unsigned)ix < (unsigned)W;
                const float v = brow[n][(size_t)(ok ? ix : 0) * Cin];
                bq[n] = ok ? v : 0.f;
            }
        };
        for (int x0 = 0; x0 < Wo; x0 += 2 * WU) {
            float a[WU][NH], bq[WU][2];
#pragma unroll
            for (int u = 0; u < WU; ++u) load(x0 + 2 * u, a[u], bq[u]);
#pragma unroll
            for (int u = 0; u < WU; ++u)
#pragma unroll
                for (int t = 0; t < NH; ++t)
#pragma unroll
                    for (int n = 0; n < 2; ++n)
                        acc[t][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][t], bq[u][n], acc[t][n], 0, 0, 0);
        }
    }
    float* out = slab + (size_t)blockIdx.z * CoP * TC;
#pragma unroll
    for (int t = 0; t < NH; ++t)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            if (!kv[n]) continue;
            const int k = (kj * 2 + n) * 32 + r;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int h = h0 + 32 * t + (e & 3) + 8 * (e >> 2) + 4 * hh;
                out[(size_t)h * TC + k] = acc[t][n][e];
            }
        }
}

// grad_w[co][c][tap] = the slabs [co][tap * Cin + c] (co < Cout of CoP rows), summed by two_level_sum; threads walk the slabs'
// own element order (whole 128-byte lines per slab) and scatter the one write.  `accum`: the value already in grad_w is added
// LAST, to the finished sum of the slabs (a caller that works through its batch in chunks: chunks in chunk order); without it
// the slabs' sum is stored as it is.  `ga`, `xa` (f16x3 slabs, conv_bwd16.hip): the |max| slots of the two operands; the finished
// sum of the slabs is scaled by 2^-(e_g + e_x) in one exact step (cp_scale_pow2) before it is stored or accumulated.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ gw, int nslab, int Cout,
                                                           int CoP, int Cin, int taps, int accum, const unsigned* __restrict__ ga,
                                                           const unsigned* __restrict__ xa) {
    __shared__ float red[256];
    float gi = 1.f, xi = 1.f, fw;
    if (ga) {
        cp_amax_to_scale(cp_amax_read(ga), &fw, &gi);
        cp_amax_to_scale(cp_amax_read(xa), &fw, &xi);
    }
    const size_t TC = (size_t)taps * Cin, n = (size_t)Cout * TC, ss = (size_t)CoP * TC;
    for (size_t base = (size_t)blockIdx.x * 32; base < n; base += (size_t)gridDim.x * 32) {  // (uniform per workgroup)
        const size_t i = base + (threadIdx.x & 31);
        float t = two_level_sum(red, i < n, nslab, 0.f, [&](float v, int s) { return v + slab[(size_t)s * ss + i]; });
        if (ga) t = cp_scale_pow2(t, gi, xi);
        if (threadIdx.x < 32 && i < n) {
            const size_t h = i / TC;
            const int k = (int)(i - h * TC), tap = k / Cin, c = k - tap * Cin;
            float* dst = gw + (h * Cin + c) * taps + tap;
            *dst = accum ? *dst + t : t;
        }
        __syncthreads();
    }
}

// Generic weight gradient: slab[s][e], e = (co, c, tap) in the PyTorch order, over the output rows of slab s, pixels ascending
__global__ void wgrad_generic_kernel(const float* __restrict__ gs, const float* __restrict__ x, float* __restrict__ slab, int rows,
                                     int Ho, int Wo, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                     int rows_per_slab) {
    const int taps = KH * KW, n = Cout * Cin * taps;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int co = e / (Cin * taps), rr = e - co * Cin * taps, c = rr / taps, t = rr - c * taps;
    const int ky = t / KW, kx = t - ky * KW;
    const int row_beg = blockIdx.y * rows_per_slab, row_end = min(rows, row_beg + rows_per_slab);
    float v = 0.f;
    for (int row = row_beg; row < row_end; ++row) {
        const int b = row / Ho, oy = row - b * Ho, iy = oy * stride + ky - pad;
        if ((unsigned)iy >= (unsigned)H) continue;
        const float* xr = x + ((size_t)b * H + iy) * W * Cin + c;
        const float* gr = gs + (size_t)row * Wo * Cout + co;
        for (int ox = 0; ox < Wo; ++ox) {
            const int ix = ox * stride + kx - pad;
            if ((unsigned)ix < (unsigned)W) v = fmaf(gr[(size_t)ox * Cout], xr[(size_t)ix * Cin], v);
        }
    }
    slab[(size_t)blockIdx.y * n + e] = v;
}

__global__ void slab_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out, int nslab, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    out[e] = serial_sum(slab, nslab, n, e, 0.f);
}

// Generic data gradient, gather form: one thread per grad_x element; taps in (ky, kx) order, output channels ascending
__global__ void dgrad_generic_kernel(const float* __restrict__ gs, const float* __restrict__ w, float* __restrict__ gx, int B, int H,
                                     int W, int Cin, int Cout, int Ho, int Wo, int KH, int KW, int stride, int pad) {
    const size_t n = (size_t)B * H * W * Cin;
    const int taps = KH * KW;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % Cin);
        const size_t px = e / Cin;
        const int ix = (int)(px % W), iy = (int)((px / W) % H), b = (int)(px / ((size_t)W * H));
        float v = 0.f;
        for (int ky = 0; ky < KH; ++ky) {
            const int ty = iy + pad - ky;
            if (ty < 0 || ty % stride) continue;
            const int oy = ty / stride;
            if (oy >= Ho) continue;
            for (int kx = 0; kx < KW; ++kx) {
                const int tx = ix + pad - kx;
                if (tx < 0 || tx % stride) continue;
                const int ox = tx / stride;
                if (ox >= Wo) continue;
                const float* gr = gs + (((size_t)b * Ho + oy) * Wo + ox) * Cout;
                const float* wr = w + (size_t)c * taps + ky * KW + kx;
                for (int co = 0; co < Cout; ++co) v = fmaf(gr[co], wr[(size_t)co * Cin * taps], v);
            }
        }
        gx[e] = v;
    }
}

// out[c] = sum over images and pixels of g [B][C][HW]: a fixed per-thread stride and a fixed tree
__global__ __launch_bounds__(256) void rowsum_kernel(const float* __restrict__ g, float* __restrict__ out, int B, int C, int HW) {
    __shared__ float red[256];
    const int c = blockIdx.x;
    float v = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* pl = g + ((size_t)b * C + c) * HW;
        for (int e = threadIdx.x; e < HW; e += 256) v += pl[e];
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[c] = red[0];
}

// Stride-1 data gradient operand: wB[(taps - 1 - tap) * CoP + co][c] = w[co][c][tap] (buffer pre-zeroed: pad rows co >= Cout and
// pad columns c >= Cin stay zero): the data gradient is the K x K / pad K/2 convolution of grad_out with the taps mirrored and
// the channel roles swapped (1x1: one tap, its own mirror)
__global__ void pack_dgrad_kernel(const float* __restrict__ w, float* __restrict__ wB, int Cout, int CoP, int Cin, int taps, int cpad) {
    const size_t n = (size_t)Cout * Cin * taps;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int co = (int)(e / ((size_t)Cin * taps));
        const int rr = (int)(e - (size_t)co * Cin * taps), c = rr / taps, t = rr - c * taps;
        wB[((size_t)(taps - 1 - t) * CoP + co) * cpad + c] = w[e];
    }
}

// Stride-2 data gradient operand: wT[tap][co][c] = w[co][c][tap] (pre-zeroed: pad rows stay zero)
__global__ void pack_dgrad_s2_kernel(const float* __restrict__ w, float* __restrict__ wT, int Cout, int CoP, int Cin, int taps) {
    const size_t n = (size_t)Cout * Cin * taps;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int co = (int)(e / ((size_t)Cin * taps));
        const int rr = (int)(e - (size_t)co * Cin * taps), c = rr / taps, t = rr - c * taps;
        wT[((size_t)t * CoP + co) * Cin + c] = w[e];
    }
}

// Stride-2 data gradient in sub-pixel form.  blockIdx.y = input pixel parity class (py, px): its pixels (2 jy + py, 2 jx + px)
// receive only the taps with ky = py + pad, kx = px + pad (mod 2), each from the grad_out pixel (jy + (py + pad - ky) / 2,
// jx + (px + pad - kx) / 2) -- for 3x3 / pad 1 that is 1, 2, 2 and 4 taps, nine in all, so no zero-inserted work; for 1x1 the
// even / even class gets the contraction and the other three write zero lines.  Per class a dense GEMM D[pixel][c] with
// K = (taps of the class) x CoP: a wave owns 2 x 32 class pixels and NT x 32 input channels.  A[pixel][k]: a lane reads 16
// bytes of its pixel's gs row (lane half = which four of eight k), B[k][c] = wT[tap][k][n0 + lane & 31]: a 128-byte line per
// half; four MFMAs pair k = j with k = 4 + j.  Halo pixels and the ragged last tile are zeros by select; the tap list is
// wave-uniform.  The results go straight into the interleaved NHWC grad_x.
template <int NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void dgrad_s2_kernel(
    const float* __restrict__ gs, const float* __restrict__ wT, float* __restrict__ gx, int B, int H, int W, int Cin, int CoP,
    int Ho, int Wo, int KK, int pad) {
    constexpr int DU = NT == 4 ? 2 : 4;
    __shared__ int opix[4][64];
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int py = blockIdx.y >> 1, px = blockIdx.y & 1;
    const int Hc = (H - py + 1) >> 1, Wc = (W - px + 1) >> 1, M = B * Hc * Wc;  // (H - py + 1) / 2 pixels of this parity
    const int NG = Cin / (32 * NT);
    const int job = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
    const int mt = job / NG, ng = job - mt * NG;
    const bool active = mt * 64 < M;  // wave-uniform
    const int n0 = ng * 32 * NT;
    // this lane's two class pixels (A rows r of the two M tiles)
    int pb[2], pjy[2], pjx[2];
    bool pv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = mt * 64 + i * 32 + r;
        pv[i] = active && m < M;
        const int mc = pv[i] ? m : 0, hw = max(Hc * Wc, 1), wc = max(Wc, 1);
        pb[i] = mc / hw;
        const int rem = mc - pb[i] * hw;
        pjy[i] = rem / wc;
        pjx[i] = rem - pjy[i] * wc;
        // the pixel's offset in grad_x (elements / Cin), shared with the lanes that store its row
        if (hh == 0) opix[wv][i * 32 + r] = pv[i] ? (pb[i] * H + 2 * pjy[i] + py) * W + 2 * pjx[i] + px : -1;
    }
    __syncthreads();
    if (!active) return;
    f32x16 acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    for (int ky = 0; ky < KK; ++ky) {
        if ((py + pad - ky) & 1) continue;  // wave-uniform
        const int oyo = (py + pad - ky) >> 1;
        for (int kx = 0; kx < KK; ++kx) {
            if ((px + pad - kx) & 1) continue;
            const int oxo = (px + pad - kx) >> 1;
            const float* ap[2];
            bool ok[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int oy = pjy[i] + oyo, ox = pjx[i] + oxo;
                ok[i] = pv[i] && (unsigned)oy < (unsigned)Ho && (unsigned)ox < (unsigned)Wo;
                ap[i] = gs + (ok[i] ? (((size_t)pb[i] * Ho + oy) * Wo + ox) * CoP : 0) + 4 * hh;
            }
            const float* bp = wT + (size_t)(ky * KK + kx) * CoP * Cin + (size_t)(4 * hh) * Cin + n0 + r;
            auto load = [&](int k0, float4 (&a)[2], float (&bq)[4][NT]) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float4 v = ld4(ap[i] + k0);
                    a[i] = ok[i] ? v : zero4();
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int t = 0; t < NT; ++t) bq[j][t] = bp[(size_t)(k0 + j) * Cin + 32 * t];
            };
            // DU steps of eight k per chunk, all requested before the chunk's first MFMA (CoP % 32 == 0: whole chunks)
            for (int k0 = 0; k0 < CoP; k0 += 8 * DU) {
                float4 a[DU][2];
                float bq[DU][4][NT];
#pragma unroll
                for (int u = 0; u < DU; ++u) load(k0 + 8 * u, a[u], bq[u]);
#pragma unroll
                for (int u = 0; u < DU; ++u) {
                    const float av[2][4] = {{a[u][0].x, a[u][0].y, a[u][0].z, a[u][0].w}, {a[u][1].x, a[u][1].y, a[u][1].z, a[u][1].w}};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int t = 0; t < NT; ++t)
                                acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][j], bq[u][j][t], acc[i][t], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int o = opix[wv][i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh];
            if (o < 0) continue;
            float* dst = gx + (size_t)o * Cin + n0 + r;
#pragma unroll
            for (int t = 0; t < NT; ++t) dst[32 * t] = acc[i][t][e];
        }
}

inline int nh_of(int c) { return c % 128 == 0 ? 4 : c % 64 == 0 ? 2 : 1; }

// Weight-gradient slabs of whole output rows: `ns` of them wanted, at most 64 MiB and at most one per row
ConvWgradPlan slab_plan(size_t rows, size_t ns, size_t wbytes, int jobs) {
    ns = std::min(ns, std::max<size_t>(1, ((size_t)64 << 20) / wbytes));
    ns = std::max<size_t>(1, std::min(ns, rows));
    ConvWgradPlan P;
    P.jobs = jobs;
    P.rows_per_slab = (int)((rows + ns - 1) / ns);
    P.slabs = (int)((rows + P.rows_per_slab - 1) / P.rows_per_slab);
    P.slab_bytes = ns * wbytes;  // (the slab count's upper bound: monotone in rows)
    return P;
}

struct Plan {
    int path;  // CP_CONV_BWD_*
    bool mfma;
    int Ho, Wo, CoP, taps;
    int st_ct, st_px, st_slabs, st_bound;  // stage_kernel: channel lanes, pixels per slab, slabs and their upper bound
    ConvWgradPlan wg;                      // weight gradient, MFMA and generic path
    ConvLowcPlan lw;                       // weight gradient, low-channel path
    bool wg16, dg16;                       // f16x3 (conv_bwd16.hip): the weight gradient, the data gradient
};

Plan plan(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int precision) {
    Plan P;
    P.path = cp_conv_backward_path(B, H, W, Cin, Cout, KH, KW, stride, pad);
    P.mfma = P.path == CP_CONV_BWD_MFMA;
    P.Ho = (H + 2 * pad - KH) / stride + 1;
    P.Wo = (W + 2 * pad - KW) / stride + 1;
    P.taps = KH * KW;
    P.CoP = P.mfma ? (Cout + 31) / 32 * 32 : Cout;
    const size_t Q = (size_t)B * P.Ho * P.Wo, rows = (size_t)B * P.Ho;
    int ct = 1;
    while (ct < P.CoP && ct < 64) ct <<= 1;
    P.st_ct = ct;
    P.st_bound = (int)std::max<size_t>(1, std::min<size_t>(512, (Q + 63) / 64));
    P.st_px = (int)((Q + P.st_bound - 1) / P.st_bound);
    P.st_slabs = (int)((Q + P.st_px - 1) / P.st_px);
    P.wg = P.mfma ? cp_conv_wgrad_plan(rows, Cin, P.CoP, P.taps) : slab_plan(rows, 64, (size_t)P.CoP * P.taps * Cin * 4, 0);
    P.lw = ConvLowcPlan{};
    if (P.path == CP_CONV_BWD_LOWC) {
        // the larger of the two plans' slab buffers: the query stays monotone in B across the path's pixel floor
        P.lw = cp_conv_lowc_wgrad_plan(B, P.Ho, P.Wo, stride);
        P.wg.slab_bytes = std::max(P.wg.slab_bytes, cp_conv_lowc_slab_bytes(B, P.Ho, P.Wo, Cout, stride));
    }
    // f16x3: the MFMA path only; a stride-1 data gradient igemm16.hip cannot take (byte offsets past 32 bits) stays float32
    P.wg16 = P.mfma && precision == CP_PREC_F16X3;
    P.dg16 = P.wg16 && (stride == 2 || cp_conv_dgrad16_s1_supported(B, H, W, Cin, P.CoP, KH));
    return P;
}

struct Ws {
    float *gs, *part, *slab, *wB;
    // f16x3: the |max| slot block (slot 0: gs, slot 1: x) and the split copies of gs and x
    unsigned* slot;
    uint32_t *gs16, *x16;
};
Ws conv_bwd_carve(Carve& c, const Plan& P, int B, int H, int W, int Cin, int stride, bool need_gx) {
    Ws r;
    const size_t gsb = (size_t)B * P.Ho * P.Wo * P.CoP * 4;
    r.gs = c.take<float>(gsb);
    r.part = c.take<float>((size_t)P.st_bound * P.CoP * 4);  // (the slab count's upper bound: monotone in B)
    r.slab = c.take<float>(P.wg.slab_bytes);
    r.wB = c.take<float>(!need_gx || !P.mfma ? 0
                         : P.dg16            ? cp_conv_dgrad16_pack_bytes(Cin, P.CoP, P.taps, stride)
                         : stride == 1       ? cp_conv_dgrad_pack_bytes(Cin, P.CoP, P.taps, CP_PREC_F32)
                                             : (size_t)P.CoP * P.taps * Cin * 4);
    r.slot = nullptr;
    r.gs16 = r.x16 = nullptr;
    if (P.wg16) {  // (nothing is taken in float32: that workspace is the one it always was)
        r.slot = c.take<unsigned>((size_t)CP_AMAX_SUB * CP_AMAX_STRIDE * sizeof(unsigned));
        r.gs16 = c.take<uint32_t>(gsb);
        // (a 1x1 layer reads each x element once: its weight gradient splits x in registers, no copy)
        r.x16 = c.take<uint32_t>(P.taps > 1 ? (size_t)B * H * W * Cin * 4 : 0);
    }
    return r;
}

}  // namespace

bool cp_conv_backward_mfma(int Cin, int KH, int KW, int stride, int pad) {
    return KH == KW && (KH == 1 || KH == 3) && (stride == 1 || stride == 2) && pad == KH / 2 && Cin % 32 == 0;
}

// The pixel floor: below it a plan of hundreds of slabs is waste, and the generic kernels cost microseconds
bool cp_conv_backward_lowc(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    if (KH != 3 || KW != 3 || pad != 1 || (stride != 1 && stride != 2) || Cin != 16 || (Cout != 16 && Cout != 32)) return false;
    const long long Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    return B * Ho * Wo >= 4096;
}

int cp_conv_backward_path(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    if (cp_conv_backward_mfma(Cin, KH, KW, stride, pad)) return CP_CONV_BWD_MFMA;
    return cp_conv_backward_lowc(B, H, W, Cin, Cout, KH, KW, stride, pad) ? CP_CONV_BWD_LOWC : CP_CONV_BWD_GENERIC;
}

// about two waves per SIMD, at most 512 slabs
ConvWgradPlan cp_conv_wgrad_plan(size_t rows, int Cin, int CoP, int taps) {
    const int KT = taps * Cin / 32, jobs = (CoP / (32 * nh_of(CoP))) * ((KT + 1) / 2);
    return slab_plan(rows, std::min<size_t>(512, (2048 + jobs - 1) / jobs), (size_t)CoP * taps * Cin * 4, jobs);
}

int cp_launch_conv_wgrad(hipStream_t s, const ConvBwdArgs& a, const float* gs, int CoP, const ConvWgradPlan& P, float* slab,
                         int accum, const ConvWgrad16* h) {
    const int Ho = (a.H + 2 * a.pad - a.KH) / a.stride + 1, Wo = (a.W + 2 * a.pad - a.KW) / a.stride + 1;
    const int taps = a.KH * a.KW, rows = a.B * Ho, slabs = (rows + P.rows_per_slab - 1) / P.rows_per_slab;
    const dim3 wg((P.jobs + 3) / 4, 1, slabs);
#define CP_WGRAD(NH)                                                                                                            \
    hipLaunchKernelGGL(wgrad_kernel<NH>, wg, dim3(256), 0, s, gs, a.x, slab, rows, Ho, Wo, a.H, a.W, a.Cin, CoP, a.KW, taps, a.stride, \
                       a.pad, P.rows_per_slab)
    if (h) {
        const int rc = cp_launch_conv_wgrad16_slabs(s, a, *h, CoP, P, slab);
        if (rc != CP_OK) return rc;
    } else {
        switch (nh_of(CoP)) {
            case 4: CP_WGRAD(4); break;
            case 2: CP_WGRAD(2); break;
            default: CP_WGRAD(1);
        }
    }
#undef CP_WGRAD
    if (!launch_ok()) return CP_ERR_LAUNCH;
    const size_t rg = std::min<size_t>(((size_t)a.Cout * taps * a.Cin + 31) / 32, 8192);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)rg), dim3(256), 0, s, (const float*)slab, a.gw, slabs, a.Cout, CoP, a.Cin,
                       taps, accum, h ? h->gs_amax : (const unsigned*)nullptr, h ? h->x_amax : (const unsigned*)nullptr);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

// wB [taps CoP][cpad], cpad = Cin rounded up to the N tile of the convolution that reads it
static int dgrad_cpad(int Cin) { return (int)cp_engine::align_up((size_t)Cin, cp_conv_tile_n(Cin)); }

size_t cp_conv_dgrad_pack_bytes(int Cin, int CoP, int taps, int precision) {
    return precision == CP_PREC_F16X3 ? cp_conv_dgrad16_pack_bytes(Cin, CoP, taps, 1) : (size_t)taps * CoP * dgrad_cpad(Cin) * 4;
}

int cp_launch_conv_dgrad_pack(hipStream_t s, const float* w, float* wB, int Cin, int Cout, int CoP, int taps, int precision) {
    if (precision == CP_PREC_F16X3) return cp_launch_conv_dgrad16_pack(s, w, wB, Cin, Cout, CoP, taps, 1);
    if (hipMemsetAsync(wB, 0, cp_conv_dgrad_pack_bytes(Cin, CoP, taps, CP_PREC_F32), s) != hipSuccess) return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(pack_dgrad_kernel, dim3(256), dim3(256), 0, s, w, wB, Cout, CoP, Cin, taps, dgrad_cpad(Cin));
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_conv_dgrad_s1(hipStream_t s, const ConvBwdArgs& a, const float* gs, int CoP, const float* wB, const float* res,
                            const unsigned* gs_amax) {
    if (gs_amax) return cp_launch_conv_dgrad16_s1(s, a, gs, CoP, wB, res, gs_amax);
    // (stride 1, pad K / 2: the output grid is the input grid, and the operand is a [a.Cin][CoP][KH][KW] weight)
    ConvParams d = grad_conv_params(a.B, a.H, a.W, gs, CoP, (float*)wB, nullptr, a.Cin, a.KH, a.KW, 1, a.pad, a.gx);
    d.res = res;
    d.res_ld = a.Cin;
    return cp_launch_conv(d, s);
}

int cp_launch_rowsum_nchw(const float* g, float* out, int B, int C, int HW, hipStream_t s) {
    hipLaunchKernelGGL(rowsum_kernel, dim3(C), dim3(256), 0, s, g, out, B, C, HW);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

size_t cp_conv_backward_ws_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int need_grad_x,
                                 int precision) {
    Carve c{nullptr};
    conv_bwd_carve(c, plan(B, H, W, Cin, Cout, KH, KW, stride, pad, precision), B, H, W, Cin, stride, need_grad_x != 0);
    return c.off;
}

int cp_conv_backward_prec_mask(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int precision) {
    const Plan P = plan(B, H, W, Cin, Cout, KH, KW, stride, pad, precision);
    return (P.wg16 ? 1 : 0) | (P.dg16 ? 2 : 0);
}

int cp_launch_conv_backward(hipStream_t s, const ConvBwdArgs& a, void* ws, int precision) {
    const Plan P = plan(a.B, a.H, a.W, a.Cin, a.Cout, a.KH, a.KW, a.stride, a.pad, precision);
    Carve cv{(char*)ws};
    const Ws r = conv_bwd_carve(cv, P, a.B, a.H, a.W, a.Cin, a.stride, a.gx != nullptr);
    float *gsb = r.gs, *part = r.part, *slab = r.slab, *wB = r.wB;
    const int B = a.B, H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout, Ho = P.Ho, Wo = P.Wo, CoP = P.CoP, taps = P.taps;
    const int Q = B * Ho * Wo, rows = B * Ho;
    // 0. stage: gate, pad, bias partials
    const bool staged = a.y || CoP != Cout;
    const float* gs = staged ? gsb : a.go;
    if (staged || a.gb) {
        hipLaunchKernelGGL(stage_kernel, dim3(P.st_slabs, (CoP + P.st_ct - 1) / P.st_ct), dim3(256), 0, s, a.go, a.y, staged ? gsb : (float*)nullptr,
                           a.gb ? part : (float*)nullptr, Q, Cout, CoP, P.st_ct, P.st_px);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        if (a.gb) {
            hipLaunchKernelGGL(bias_reduce_kernel, dim3((Cout + 31) / 32), dim3(256), 0, s, (const float*)part, a.gb,
                               P.st_slabs, Cout, CoP);
            if (!launch_ok()) return CP_ERR_LAUNCH;
        }
    }
    // f16x3: the |max| of gs and x, then their split copies (the gate, the pad lanes and grad_bias above stay float32)
    const unsigned *g_amax = r.slot, *x_amax = r.slot + 1;
    if (P.wg16) {
        const size_t ng = (size_t)Q * CoP, nx = (size_t)B * H * W * Cin;
        if (hipMemsetAsync(r.slot, 0, (size_t)CP_AMAX_SUB * CP_AMAX_STRIDE * sizeof(unsigned), s) != hipSuccess) return CP_ERR_LAUNCH;
        int rc = cp_launch_absmax32(gs, ng, r.slot, s);
        if (rc == CP_OK) rc = cp_launch_absmax32(a.x, nx, r.slot + 1, s);
        if (rc == CP_OK) rc = cp_launch_split16(gs, r.gs16, ng, g_amax, s);
        if (rc == CP_OK && taps > 1) rc = cp_launch_split16(a.x, r.x16, nx, x_amax, s);
        if (rc != CP_OK) return rc;
    }
    // 1. grad_w
    if (P.mfma) {
        const ConvWgrad16 h{r.gs16, taps > 1 ? r.x16 : nullptr, g_amax, x_amax};
        const int rc = cp_launch_conv_wgrad(s, a, gs, CoP, P.wg, slab, 0, P.wg16 ? &h : nullptr);
        if (rc != CP_OK) return rc;
    } else if (P.path == CP_CONV_BWD_LOWC) {
        const int rc = cp_launch_conv_lowc_wgrad(s, a, gs, P.lw, slab);
        if (rc != CP_OK) return rc;
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((Cout * taps * Cin + 31) / 32), dim3(256), 0, s, (const float*)slab, a.gw,
                           P.lw.wgs, Cout, CoP, Cin, taps, 0, (const unsigned*)nullptr, (const unsigned*)nullptr);
        if (!launch_ok()) return CP_ERR_LAUNCH;
    } else {
        const int n = Cout * Cin * taps;
        hipLaunchKernelGGL(wgrad_generic_kernel, dim3((n + 255) / 256, P.wg.slabs), dim3(256), 0, s, gs, a.x, slab, rows, Ho, Wo, H,
                           W, Cin, Cout, a.KH, a.KW, a.stride, a.pad, P.wg.rows_per_slab);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        hipLaunchKernelGGL(slab_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const float*)slab, a.gw, P.wg.slabs, n);
        if (!launch_ok()) return CP_ERR_LAUNCH;
    }
    // 2. grad_x
    if (!a.gx) return CP_OK;
    if (P.path == CP_CONV_BWD_LOWC) return cp_launch_conv_lowc_dgrad(s, a, gs);
    if (!P.mfma) {
        const size_t n = (size_t)B * H * W * Cin;
        hipLaunchKernelGGL(dgrad_generic_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 65536)), dim3(256), 0, s, gs, a.w,
                           a.gx, B, H, W, Cin, Cout, Ho, Wo, a.KH, a.KW, a.stride, a.pad);
        return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
    }
    if (a.stride == 1) {
        const int rc = cp_launch_conv_dgrad_pack(s, a.w, wB, Cin, Cout, CoP, taps, P.dg16 ? CP_PREC_F16X3 : CP_PREC_F32);
        return rc != CP_OK ? rc : cp_launch_conv_dgrad_s1(s, a, gs, CoP, wB, nullptr, P.dg16 ? g_amax : nullptr);
    }
    if (P.dg16) {
        const int rc = cp_launch_conv_dgrad16_pack(s, a.w, wB, Cin, Cout, CoP, taps, 2);
        return rc != CP_OK ? rc : cp_launch_conv_dgrad16_s2(s, a, r.gs16, CoP, wB, g_amax);
    }
    if (hipMemsetAsync(wB, 0, (size_t)CoP * taps * Cin * 4, s) != hipSuccess) return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(pack_dgrad_s2_kernel, dim3(256), dim3(256), 0, s, a.w, wB, Cout, CoP, Cin, taps);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    const int M0 = B * ((H + 1) / 2) * ((W + 1) / 2);  // the even / even class has the most pixels
    const int nt = nh_of(Cin), jobs = ((M0 + 63) / 64) * (Cin / (32 * nt));
    const dim3 dg((jobs + 3) / 4, 4);
#define CP_DGRAD(NT) \
    hipLaunchKernelGGL(dgrad_s2_kernel<NT>, dg, dim3(256), 0, s, gs, (const float*)wB, a.gx, B, H, W, Cin, CoP, Ho, Wo, a.KH, a.pad)
    switch (nt) {
        case 4: CP_DGRAD(4); break;
        case 2: CP_DGRAD(2); break;
        default: CP_DGRAD(1);
    }
#undef CP_DGRAD
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
