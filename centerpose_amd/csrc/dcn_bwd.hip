// DCNv2 backward (cp_dcnv2_backward): the input, offset, mask, weight and bias gradients of the modulated deformable
// convolution, with the semantics of the reference's CUDA op (DCNv2/src/cuda/
// dcn_v2_cuda.cu:206-340 and the col2im / col2im_coord kernels of dcn_v2_im2col_cuda.cu:197-327), quirks included.
//
// Index: k = tap * C + c throughout (tap = i * kw + j), against the reference's c * kh * kw + tap; the weight is
// re-ordered once.  Launch sequence per call (all on the caller's stream, float32 arithmetic only):
//   1. wt[co][k] = weight[co][c][tap]; go_t = grad_output as [B*Ho*Wo][Co]; fast path: x staged NHWC, the NHWC input
//      gradient zeroed (generic path: the caller's grad_input zeroed).
//   2. per chunk of `nb` images:
//      gcol_kernel  grad_col[b][k][pix] = sum_co wt[co][k] * go[b][co][pix]  (v_mfma_f32_32x32x2_f32, co ascending);
//      data kernel  per sample (b, group, tap, pixel), channels ascending in one lane:
//                     grad_offset (h, w) = sum_c coord_weight(x) * grad_col * mask    (col2im_coord, :256-327)
//                     grad_mask          = sum_c grad_col * bilinear(x)
//                     grad_input        += bilinear weight * grad_col * mask at the in-image corners (col2im, :197-254)
//                   fast path (dcn_bwd_halo_kernel): a 16 x 4 pixel patch x 9 taps per workgroup, the corner adds of a
//                   channel chunk go to an LDS halo tile around the patch (float LDS atomics); only corners outside it
//                   are global atomics; the tile is flushed with one global atomic per non-zero (cell, channel).
//                   generic path (dcn_bwd_generic_kernel): one lane per sample, corner adds straight to NCHW global.
//   3. wgrad_kernel  slab[s][co][k] = sum over the pixels of slab s of go_t[q][co] * col[q][k], col = the forward's
//      modulated im2col computed in the B operand's lane (v_mfma_f32_32x32x2_f32, pixels ascending);
//      wgrad_reduce_kernel sums the slabs in slab order; cp_launch_rowsum_nchw sums grad_output per channel in a fixed tree.
//   4. fast path: the NHWC input gradient back to NCHW.
// grad_offset, grad_mask, grad_weight and grad_bias are bitwise reproducible (every sum has a fixed order); grad_input
// is summed with float atomics, so its last bits depend on arrival order.
//
// cp_dcnv2_backward_det (fast geometry only) replaces step 2's data kernel by an inverted index: grad_col is stored
// pixel-major, every (pixel, tap, corner) is sorted by its destination cell, and each cell sums its own list in a fixed
// order with plain stores -- grad_input is then bitwise reproducible as well (see "the deterministic input gradient" below
// and the contract in include/centerpose_hip.h).
//
// CP_PREC_F16X3 (cp_dcnv2_backward_prec; fast geometry, both forms): the two contractions run in split binary16 (dcn_bwd16.hip).
//   1'. go_t becomes [B*Ho*Wo][CoP] with zeroed pad lanes (CoP = Co rounded up to 32), its |max|, |max x| and |max mask| go to
//       three slots of one block, go16 = split(go_t); wt is packed as the data gradient's operand of the 1x1 convolution 9C -> Co.
//   2'. per chunk: grad_col[b][pix][k], pixel-major on BOTH forms, = that convolution's stride-1 data gradient
//       (cp_launch_conv_dgrad16_s1; gcol_kernel<true> where cp_conv_dgrad16_s1_supported refuses the chunk); the halo kernel reads
//       it through its PM flag; col16 = the chunk's deformable columns as split dwords; the slab kernel adds the chunk's sums.
//   3'. the slabs' two-level sum times the two inverse scales.  wgrad_kernel does not run.
// grad_col and col16 of a chunk each follow the 256 MiB rule, so the chunks are the float32 mode's.
#include "op_common.h"
#include "igemm_common.h"
#include "dcn_bwd_det_common.h"
#include "dcn_bwd_sample.h"

#include <algorithm>

namespace {

constexpr int HALO_R = 4;                  // halo margin around the 16 x 4 patch (taps reach 1, offsets the rest)
constexpr int PT_X = 16, PT_Y = 4;         // patch of output pixels per workgroup of the halo kernel
constexpr int HX = PT_X + 2 * HALO_R + 1;  // + 1: the high corner of a sample at the margin's edge
constexpr int HY = PT_Y + 2 * HALO_R + 1;
constexpr int WG_COUT = 4;                 // 32-row Co tiles per wave of the weight-gradient kernel (at most)

struct BwdP {
    const float* x;     // [B,C,H,W]
    const float* xh;    // [B,H,W,C] (fast path) or nullptr
    const float* wt;    // [Co][T*C]
    const float* off;   // [B, dg*2T, Ho, Wo]
    const float* mask;  // [B, dg*T, Ho, Wo]
    const float* go;    // [B, Co, Ho, Wo]
    const float* go_t;  // [B*Ho*Wo, Co]
    float* gcol;        // [nb][T*C][Ho*Wo]
    float* gin;         // fast: [B,H,W,C]; generic: [B,C,H,W]
    float* goff;
    float* gmask;
    float* slab;        // [nslab][Co][T*C]
    int B, C, H, W, Co, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, dg;
    int b0, nb, slab_px, nslab;
};

__global__ void wt_kernel(const float* __restrict__ w, float* __restrict__ wt, int Co, int C, int T) {
    const size_t n = (size_t)Co * C * T;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t co = e / ((size_t)C * T);
        const int r = (int)(e - co * C * T), c = r / T, t = r - c * T;
        wt[co * C * T + (size_t)t * C + c] = w[e];
    }
}

// grad_col of images b0 .. b0+nb-1: D[k][pix] over K = Co.  A[k][co] = wt[co][k], B[co][pix] = go[b][co][pix].
// A workgroup of 4 waves owns 128 k x 128 pixels; each wave 64 x 64 (2 x 2 accumulators).  PM: the deterministic path's
// pixel-major store grad_col[b][pix][k] (a lane's accumulator holds four consecutive k: one 16-byte store; T*C % 4 == 0 there).
template <bool PM>
__global__ __launch_bounds__(256) void gcol_kernel(const BwdP p) {
    const int TC = p.C * p.kh * p.kw, HWo = p.Ho * p.Wo;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k0 = blockIdx.y * 128 + (wv >> 1) * 64, px0 = blockIdx.x * 128 + (wv & 1) * 64;
    const int bi = blockIdx.z, b = p.b0 + bi;
    const int r = lane & 31, h = lane >> 5;
    const float* go = p.go + (size_t)b * p.Co * HWo;
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
    const bool ka0 = k0 + r < TC, ka1 = k0 + 32 + r < TC;
    const bool pb0 = px0 + r < HWo, pb1 = px0 + 32 + r < HWo;
    for (int c2 = 0; c2 < p.Co; c2 += 2) {  // uniform over the wave; lane half h takes co = c2 + h
        const int co = c2 + h;
        const bool cv = co < p.Co;
        const float* wr = p.wt + (size_t)(cv ? co : 0) * TC;
        const float* gr = go + (size_t)(cv ? co : 0) * HWo;
        const float a0 = (cv && ka0) ? wr[k0 + r] : 0.f;
        const float a1 = (cv && ka1) ? wr[k0 + 32 + r] : 0.f;
        const float b0v = (cv && pb0) ? gr[px0 + r] : 0.f;
        const float b1v = (cv && pb1) ? gr[px0 + 32 + r] : 0.f;
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0v, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1v, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0v, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1v, acc[1][1], 0, 0, 0);
    }
    float* out = p.gcol + (size_t)bi * TC * HWo;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int px = px0 + 32 * n + r;
            if (px >= HWo) continue;
            if (PM) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int k = k0 + 32 * m + 8 * g + 4 * h;
                    if (k < TC)
                        *reinterpret_cast<float4*>(out + (size_t)px * TC + k) =
                            make_float4(acc[m][n][4 * g], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]);
                }
                continue;
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int k = k0 + 32 * m + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (k < TC) out[(size_t)k * HWo + px] = acc[m][n][e];
            }
        }
}

// fast path: 3x3, stride 1, pad 1, dilation 1, one deformable group, C % CH == 0; x and the input gradient NHWC.
// 9 waves: wave = tap, lane = pixel of the 16 x 4 patch.  PM: grad_col is pixel-major [b][pix][k] (the f16x3 mode's data gradient
// stores it so): a lane reads its four channels as one 16-byte piece.
template <int CH, bool PM>
__global__ __launch_bounds__(576) void dcn_bwd_halo_kernel(const BwdP p) {
    __shared__ float halo[HY * HX * (CH + 1)];  // + 1: cells of one channel fall in different banks
    const int C = p.C, H = p.H, W = p.W, HWo = p.Ho * p.Wo, TC = 9 * C;
    const int tap = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ty0 = blockIdx.y * PT_Y, tx0 = blockIdx.x * PT_X;
    const int ho = ty0 + (lane >> 4), wo = tx0 + (lane & 15);
    const int bi = blockIdx.z, b = p.b0 + bi;
    const bool act = ho < p.Ho && wo < p.Wo;
    const int pix = act ? ho * p.Wo + wo : 0;
    const int hy0 = ty0 - HALO_R, hx0 = tx0 - HALO_R;
    const int i = tap / 3, j = tap - 3 * i;
    const float oh = act ? p.off[((size_t)b * 18 + 2 * tap) * HWo + pix] : 0.f;
    const float ow = act ? p.off[((size_t)b * 18 + 2 * tap + 1) * HWo + pix] : 0.f;
    const float m = act ? p.mask[((size_t)b * 9 + tap) * HWo + pix] : 0.f;
    const Sample s = make_sample((float)(ho - 1 + i) + oh, (float)(wo - 1 + j) + ow, H, W);
    const bool live = act && s.in;
    const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
    // corner cells in the halo tile (-1: outside it, the add goes to global memory)
    int cell[4];
    size_t gaddr[4];
    bool cv[4] = {s.c1 && live, s.c2 && live, s.c3 && live, s.c4 && live};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int y = s.y0 + (q >> 1), x = s.x0 + (q & 1);
        const int ly = y - hy0, lx = x - hx0;
        cell[q] = (ly >= 0 && ly < HY && lx >= 0 && lx < HX) ? ly * HX + lx : -1;
        gaddr[q] = cv[q] ? (((size_t)b * H + y) * W + x) * C : 0;
    }
    const float* xb = p.xh;
    const float* gc = PM ? p.gcol + ((size_t)bi * HWo + pix) * TC + (size_t)tap * C
                         : p.gcol + ((size_t)bi * TC + (size_t)tap * C) * HWo + pix;
    float vh = 0.f, vw = 0.f, mv = 0.f;
    for (int c0 = 0; c0 < C; c0 += CH) {
        for (int e = threadIdx.x; e < HY * HX * (CH + 1); e += 576) halo[e] = 0.f;
        __syncthreads();
        if (live) {
            for (int cc = 0; cc < CH; cc += 4) {
                const int c = c0 + cc;
                const float4 v1 = cv[0] ? ld4(xb + gaddr[0] + c) : zero4();
                const float4 v2 = cv[1] ? ld4(xb + gaddr[1] + c) : zero4();
                const float4 v3 = cv[2] ? ld4(xb + gaddr[2] + c) : zero4();
                const float4 v4 = cv[3] ? ld4(xb + gaddr[3] + c) : zero4();
                const float a1[4] = {v1.x, v1.y, v1.z, v1.w}, a2[4] = {v2.x, v2.y, v2.z, v2.w};
                const float a3[4] = {v3.x, v3.y, v3.z, v3.w}, a4[4] = {v4.x, v4.y, v4.z, v4.w};
                const float4 g4 = PM ? ld4(gc + c) : zero4();
                const float ga[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float g = PM ? ga[u] : gc[(size_t)(c + u) * HWo];
                    const float cwh = -s.hw * a1[u] - s.lw * a2[u] + s.hw * a3[u] + s.lw * a4[u];
                    const float cww = -s.hh * a1[u] + s.hh * a2[u] - s.lh * a3[u] + s.lh * a4[u];
                    vh += cwh * g * m;
                    vw += cww * g * m;
                    mv += g * (w1 * a1[u] + w2 * a2[u] + w3 * a3[u] + w4 * a4[u]);
                    const float gm = g * m;
                    const float add[4] = {w1 * gm, w2 * gm, w3 * gm, w4 * gm};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (!cv[q]) continue;
                        if (cell[q] >= 0)
                            atomicAdd(&halo[cell[q] * (CH + 1) + cc + u], add[q]);
                        else
                            atomicAdd(p.gin + gaddr[q] + c + u, add[q]);
                    }
                }
            }
        }
        __syncthreads();
        // flush: one global add per non-zero (cell, channel) inside the image; lanes run along the channels
        for (int e = threadIdx.x; e < HY * HX * CH; e += 576) {
            const int cl = e / CH, cc = e - cl * CH;
            const int ly = cl / HX, lx = cl - ly * HX;
            const int y = hy0 + ly, x = hx0 + lx;
            const float v = halo[cl * (CH + 1) + cc];
            if (y >= 0 && y < H && x >= 0 && x < W && v != 0.f)
                atomicAdd(p.gin + (((size_t)b * H + y) * W + x) * C + c0 + cc, v);
        }
        __syncthreads();
    }
    if (act) {
        p.goff[((size_t)b * 18 + 2 * tap) * HWo + pix] = vh;
        p.goff[((size_t)b * 18 + 2 * tap + 1) * HWo + pix] = vw;
        p.gmask[((size_t)b * 9 + tap) * HWo + pix] = mv;
    }
}

// generic path: any kernel / stride / padding / dilation / deformable_group / C; NCHW throughout.  One lane per
// sample (image of the chunk, group, tap, pixel).  The input gradient's sample uses pad_h on both axes, as the reference's
// launchers do (dcn_v2_im2col_cuda.cu:368, dcn_v2_im2col_cpu.cpp:364); offsets and masks use (pad_h, pad_w).
__global__ __launch_bounds__(256) void dcn_bwd_generic_kernel(const BwdP p) {
    const int T = p.kh * p.kw, HWo = p.Ho * p.Wo, TC = p.C * T, cpg = p.C / p.dg;
    const size_t n = (size_t)p.nb * p.dg * T * HWo;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int pix = (int)(e % HWo);
        size_t r = e / HWo;
        const int tap = (int)(r % T);
        r /= T;
        const int g = (int)(r % p.dg);
        const int bi = (int)(r / p.dg), b = p.b0 + bi;
        const int ho = pix / p.Wo, wo = pix - ho * p.Wo;
        const int i = tap / p.kw, j = tap - i * p.kw;
        const size_t ob = ((size_t)b * p.dg + g) * 2 * T;
        const float oh = p.off[(ob + 2 * tap) * HWo + pix], ow = p.off[(ob + 2 * tap + 1) * HWo + pix];
        const size_t mi = (((size_t)b * p.dg + g) * T + tap) * HWo + pix;
        const float m = p.mask[mi];
        const float sy = (float)(ho * p.sh - p.ph + i * p.dh) + oh;
        const Sample s = make_sample(sy, (float)(wo * p.sw - p.pw + j * p.dw) + ow, p.H, p.W);
        const Sample t = make_sample(sy, (float)(wo * p.sw - p.ph + j * p.dw) + ow, p.H, p.W);  // the col2im quirk
        const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
        const float t1 = t.hh * t.hw, t2 = t.hh * t.lw, t3 = t.lh * t.hw, t4 = t.lh * t.lw;
        float vh = 0.f, vw = 0.f, mv = 0.f;
        for (int cl = 0; cl < cpg; ++cl) {
            const int c = g * cpg + cl;
            const float gv = p.gcol[((size_t)bi * TC + (size_t)tap * p.C + c) * HWo + pix];
            const size_t plane = ((size_t)b * p.C + c) * p.H * p.W;
            if (s.in) {
                const float* xp = p.x + plane;
                const float a1 = s.c1 ? xp[(size_t)s.y0 * p.W + s.x0] : 0.f;
                const float a2 = s.c2 ? xp[(size_t)s.y0 * p.W + s.x0 + 1] : 0.f;
                const float a3 = s.c3 ? xp[(size_t)(s.y0 + 1) * p.W + s.x0] : 0.f;
                const float a4 = s.c4 ? xp[(size_t)(s.y0 + 1) * p.W + s.x0 + 1] : 0.f;
                vh += (-s.hw * a1 - s.lw * a2 + s.hw * a3 + s.lw * a4) * gv * m;
                vw += (-s.hh * a1 + s.hh * a2 - s.lh * a3 + s.lh * a4) * gv * m;
                mv += gv * (w1 * a1 + w2 * a2 + w3 * a3 + w4 * a4);
            }
            if (t.in) {
                const float gm = gv * m;
                float* gp = p.gin + plane;
                if (t.c1) atomicAdd(gp + (size_t)t.y0 * p.W + t.x0, t1 * gm);
                if (t.c2) atomicAdd(gp + (size_t)t.y0 * p.W + t.x0 + 1, t2 * gm);
                if (t.c3) atomicAdd(gp + (size_t)(t.y0 + 1) * p.W + t.x0, t3 * gm);
                if (t.c4) atomicAdd(gp + (size_t)(t.y0 + 1) * p.W + t.x0 + 1, t4 * gm);
            }
        }
        p.goff[(ob + 2 * tap) * HWo + pix] = vh;
        p.goff[(ob + 2 * tap + 1) * HWo + pix] = vw;
        p.gmask[mi] = mv;
    }
}

// slab[s][co][k] = sum_{q in slab s} go_t[q][co] * col(q, k): D[co][k] over K = pixels, 2 per MFMA step.  A wave owns
// 32 k columns and NCO 32-row Co tiles; lane l builds col(q0 + (l >> 5), k0 + (l & 31)) itself.
template <int NCO>
__global__ __launch_bounds__(256) void wgrad_kernel(const BwdP p) {
    const int T = p.kh * p.kw, TC = p.C * T, HWo = p.Ho * p.Wo, cpg = p.C / p.dg;
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int k0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    if (k0 >= TC) return;
    const int co0 = blockIdx.y * 32 * NCO;
    const int sl = blockIdx.z;
    const int Q = p.B * HWo;
    const int q_beg = sl * p.slab_px, q_end = min(Q, q_beg + p.slab_px);
    const int k = k0 + r;
    const bool kv = k < TC;
    const int tap = kv ? k / p.C : 0, c = kv ? k - tap * p.C : 0;
    const int i = tap / p.kw, j = tap - i * p.kw;
    const int g = c / cpg;
    f32x16 acc[NCO];
#pragma unroll
    for (int t = 0; t < NCO; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    for (int q0 = q_beg; q0 < q_end; q0 += 2) {
        const int q = q0 + h;
        const bool qv = q < q_end;
        float bv = 0.f;
        if (qv && kv) {
            const int b = q / HWo, pix = q - b * HWo;
            const int ho = pix / p.Wo, wo = pix - ho * p.Wo;
            const size_t ob = ((size_t)b * p.dg + g) * 2 * T;
            const float oh = p.off[(ob + 2 * tap) * HWo + pix], ow = p.off[(ob + 2 * tap + 1) * HWo + pix];
            const float m = p.mask[(((size_t)b * p.dg + g) * T + tap) * HWo + pix];
            const Sample s = make_sample((float)(ho * p.sh - p.ph + i * p.dh) + oh,
                                         (float)(wo * p.sw - p.pw + j * p.dw) + ow, p.H, p.W);
            float a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
            if (p.xh) {
                const float* xb = p.xh + (size_t)b * p.H * p.W * p.C + c;
                if (s.c1) a1 = xb[((size_t)s.y0 * p.W + s.x0) * p.C];
                if (s.c2) a2 = xb[((size_t)s.y0 * p.W + s.x0 + 1) * p.C];
                if (s.c3) a3 = xb[((size_t)(s.y0 + 1) * p.W + s.x0) * p.C];
                if (s.c4) a4 = xb[((size_t)(s.y0 + 1) * p.W + s.x0 + 1) * p.C];
            } else {
                const float* xp = p.x + ((size_t)b * p.C + c) * p.H * p.W;
                if (s.c1) a1 = xp[(size_t)s.y0 * p.W + s.x0];
                if (s.c2) a2 = xp[(size_t)s.y0 * p.W + s.x0 + 1];
                if (s.c3) a3 = xp[(size_t)(s.y0 + 1) * p.W + s.x0];
                if (s.c4) a4 = xp[(size_t)(s.y0 + 1) * p.W + s.x0 + 1];
            }
            // the forward's column value: (w1 v1 + w2 v2 + w3 v3 + w4 v4) * mask, zero outside (-1, H) x (-1, W)
            const float val = (s.hh * s.hw) * a1 + (s.hh * s.lw) * a2 + (s.lh * s.hw) * a3 + (s.lh * s.lw) * a4;
            bv = s.in ? val * m : 0.f;
        }
        const float* gr = p.go_t + (size_t)(qv ? q : 0) * p.Co;
#pragma unroll
        for (int t = 0; t < NCO; ++t) {
            const int co = co0 + 32 * t + r;
            const float av = (qv && co < p.Co) ? gr[co] : 0.f;
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
        }
    }
    float* out = p.slab + (size_t)sl * p.Co * TC;
    if (!kv) return;
#pragma unroll
    for (int t = 0; t < NCO; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int co = co0 + 32 * t + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (co < p.Co) out[(size_t)co * TC + k] = acc[t][e];
        }
}

// grad_weight[co][c][tap] = the slabs' [co][tap][c] by serial_sum
__global__ void wgrad_reduce_kernel(const float* __restrict__ slab, float* __restrict__ gw, int nslab, int Co, int C, int T) {
    const size_t n = (size_t)Co * C * T, TC = (size_t)C * T;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t co = e / TC;
        const int r = (int)(e - co * TC), c = r / T, t = r - c * T;
        const size_t src = co * TC + (size_t)t * C + c;
        gw[e] = serial_sum(slab, nslab, n, src, 0.f);
    }
}

// ---- the deterministic input gradient (cp_dcnv2_backward_det; fast geometry only) ----
// Per chunk of nb images, n = nb * H * W * 36 entries (pixel, tap, corner), the entry id = its position at the start:
//   dcn_det_coord_kernel   grad_offset / grad_mask as the halo kernel sums them, from the pixel-major grad_col;
//   dcn_det_index_kernel   keys[id] = destination cell of the corner within the chunk, or `cells` where it adds nothing;
//   rs_* kernels           stable LSD radix sort of (key, id) in 8-bit digits: ids of one cell come out ascending;
//   dcn_det_rows_kernel    [begin, end) of each cell's list, by key change (cells without a list keep the memset's 0, 0);
//   dcn_det_gather_kernel  a group of lanes per cell walks the first DCN_DET_CHUNK entries of its list in order and stores
//                          the NHWC grad_input line with plain stores (zeros for an empty list);
//   dcn_det_long_kernel    further chunks of a longer list, one wave each, into partial rows;
//   dcn_det_long_add_kernel  adds a long list's partial rows to its line in chunk order.
// No float atomic anywhere: the only atomics are the radix histogram's integer counters in LDS.

struct DetP {
    uint32_t *keys, *ids;  // sorted
    uint32_t* rows;        // [cells][2]
    float* partial;        // [ceil(n / DCN_DET_CHUNK)][C]
    uint32_t n, cells;
};

// (image of the chunk, pixel, tap) of lane e = pp * 9 + tap, and its sample
struct DetTap {
    uint32_t pp;
    int tap, b, pix;
    float m;
    DcnDetSample s;
};
__device__ __forceinline__ DetTap det_tap(const BwdP& p, uint32_t e) {
    const int HW = p.H * p.W;
    DetTap t;
    t.pp = e / 9u;
    t.tap = (int)(e - t.pp * 9u);
    const int bi = (int)(t.pp / (uint32_t)HW);
    t.pix = (int)(t.pp - (uint32_t)bi * HW);
    t.b = p.b0 + bi;
    const int ho = t.pix / p.W, wo = t.pix - ho * p.W;
    const float oh = p.off[((size_t)t.b * 18 + 2 * t.tap) * HW + t.pix];
    const float ow = p.off[((size_t)t.b * 18 + 2 * t.tap + 1) * HW + t.pix];
    t.m = p.mask[((size_t)t.b * 9 + t.tap) * HW + t.pix];
    t.s = dcn_det_sample_at(ho, wo, t.tap, oh, ow, p.H, p.W);
    return t;
}

__global__ __launch_bounds__(256) void dcn_det_coord_kernel(const BwdP p) {
    const int C = p.C, HW = p.H * p.W;
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint32_t)p.nb * HW * 9u) return;
    const DetTap t = det_tap(p, e);
    const DcnDetSample& s = t.s;
    const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
    float vh = 0.f, vw = 0.f, mv = 0.f;
    if (s.in) {
        const float* xb = p.xh + (size_t)t.b * HW * C;
        const float* gc = p.gcol + (size_t)e * C;
        const float* xq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) xq[q] = xb + (s.c[q] ? ((size_t)(s.y0 + (q >> 1)) * p.W + (s.x0 + (q & 1))) * C : 0);
        for (int c = 0; c < C; c += 4) {
            const float4 v1 = s.c[0] ? ld4(xq[0] + c) : zero4();
            const float4 v2 = s.c[1] ? ld4(xq[1] + c) : zero4();
            const float4 v3 = s.c[2] ? ld4(xq[2] + c) : zero4();
            const float4 v4 = s.c[3] ? ld4(xq[3] + c) : zero4();
            const float4 g4 = ld4(gc + c);
            const float a1[4] = {v1.x, v1.y, v1.z, v1.w}, a2[4] = {v2.x, v2.y, v2.z, v2.w};
            const float a3[4] = {v3.x, v3.y, v3.z, v3.w}, a4[4] = {v4.x, v4.y, v4.z, v4.w};
            const float ga[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float g = ga[u];
                const float cwh = -s.hw * a1[u] - s.lw * a2[u] + s.hw * a3[u] + s.lw * a4[u];
                const float cww = -s.hh * a1[u] + s.hh * a2[u] - s.lh * a3[u] + s.lh * a4[u];
                vh += cwh * g * t.m;
                vw += cww * g * t.m;
                mv += g * (w1 * a1[u] + w2 * a2[u] + w3 * a3[u] + w4 * a4[u]);
            }
        }
    }
    p.goff[((size_t)t.b * 18 + 2 * t.tap) * HW + t.pix] = vh;
    p.goff[((size_t)t.b * 18 + 2 * t.tap + 1) * HW + t.pix] = vw;
    p.gmask[((size_t)t.b * 9 + t.tap) * HW + t.pix] = mv;
}

__global__ __launch_bounds__(256) void dcn_det_index_kernel(const BwdP p, uint32_t* __restrict__ keys, uint32_t* __restrict__ ids,
                                                            uint32_t cells) {
    const int HW = p.H * p.W;
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (uint32_t)p.nb * HW * 9u) return;
    const DetTap t = det_tap(p, e);
    const int bi = t.b - p.b0;
    uint4 k, i;
    k.x = dcn_det_key(t.s, 0, bi, p.H, p.W, cells), i.x = dcn_det_id(t.pp, t.tap, 0);
    k.y = dcn_det_key(t.s, 1, bi, p.H, p.W, cells), i.y = dcn_det_id(t.pp, t.tap, 1);
    k.z = dcn_det_key(t.s, 2, bi, p.H, p.W, cells), i.z = dcn_det_id(t.pp, t.tap, 2);
    k.w = dcn_det_key(t.s, 3, bi, p.H, p.W, cells), i.w = dcn_det_id(t.pp, t.tap, 3);
    reinterpret_cast<uint4*>(keys)[e] = k;
    reinterpret_cast<uint4*>(ids)[e] = i;
}

// Radix pass over the digit (key >> shift) & 255.  A tile is RS_TILE consecutive entries; hist[digit][tile] counts them,
// the rs_scan_* kernels turn the table (digit-major) into start positions, rs_scatter_kernel moves each entry to its digit's
// start + its rank among the tile's earlier entries of that digit: stable.
constexpr int RS_TILE = 4096;

__global__ __launch_bounds__(256) void rs_hist_kernel(const uint32_t* __restrict__ keys, uint32_t* __restrict__ hist, uint32_t n,
                                                      int shift, uint32_t ntiles) {
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)RS_TILE;
    for (uint32_t i = threadIdx.x; i < (uint32_t)RS_TILE; i += 256) {
        const uint32_t e = base + i;
        if (e < n) atomicAdd(&cnt[(keys[e] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}

// Exclusive scan of h[0 .. m) in place, m a multiple of 256, in two launches over segments of SCAN_SEG elements (16 per
// thread, contiguous): rs_scan_sums_kernel leaves each segment's sum, rs_scan_apply_kernel starts a segment at the sum of the
// segments before it (each workgroup adds those up itself) and scans its own.
constexpr int SCAN_SEG = 4096;

__device__ __forceinline__ uint32_t block_sum_256(uint32_t (&red)[256], uint32_t v) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    const uint32_t r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void rs_scan_sums_kernel(const uint32_t* __restrict__ h, uint32_t* __restrict__ sums, uint32_t m) {
    __shared__ uint32_t red[256];
    const uint32_t base = blockIdx.x * (uint32_t)SCAN_SEG + threadIdx.x * 16u;
    uint32_t s = 0;
    if (base < m)
        for (int i = 0; i < 4; ++i) {
            const uint4 v = reinterpret_cast<const uint4*>(h + base)[i];
            s += v.x + v.y + v.z + v.w;
        }
    const uint32_t total = block_sum_256(red, s);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void rs_scan_apply_kernel(uint32_t* __restrict__ h, const uint32_t* __restrict__ sums, uint32_t m) {
    __shared__ uint32_t red[256];
    const uint32_t t = threadIdx.x, base = blockIdx.x * (uint32_t)SCAN_SEG + t * 16u;
    uint32_t before = 0;
    for (uint32_t g = t; g < blockIdx.x; g += 256u) before += sums[g];
    before = block_sum_256(red, before);
    uint32_t v[16], s = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = 0;
    if (base < m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 q = reinterpret_cast<const uint4*>(h + base)[i];
            v[4 * i] = q.x, v[4 * i + 1] = q.y, v[4 * i + 2] = q.z, v[4 * i + 3] = q.w;
        }
#pragma unroll
    for (int i = 0; i < 16; ++i) s += v[i];
    red[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {  // inclusive scan of the threads' sums
        const uint32_t u = t >= d ? red[t - d] : 0u;
        __syncthreads();
        red[t] += u;
        __syncthreads();
    }
    uint32_t run = before + red[t] - s;
    if (base < m)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint4 q;
            q.x = run, run += v[4 * i];
            q.y = run, run += v[4 * i + 1];
            q.z = run, run += v[4 * i + 2];
            q.w = run, run += v[4 * i + 3];
            reinterpret_cast<uint4*>(h + base)[i] = q;
        }
}

// one wave per tile, 64 entries a round in entry order: the rank of an entry among the round's equal digits comes from
// ballots, the count of earlier rounds from pos[]
__global__ __launch_bounds__(64) void rs_scatter_kernel(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ ids_in,
                                                        uint32_t* __restrict__ keys_out, uint32_t* __restrict__ ids_out,
                                                        const uint32_t* __restrict__ hist, uint32_t n, int shift,
                                                        uint32_t ntiles) {
    __shared__ uint32_t pos[256];
    const uint32_t lane = threadIdx.x;
    for (uint32_t d = lane; d < 256u; d += 64u) pos[d] = hist[d * ntiles + blockIdx.x];
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)RS_TILE;
    for (uint32_t r = 0; r < (uint32_t)RS_TILE; r += 64u) {
        const uint32_t e = base + r + lane;
        const bool valid = e < n;
        const uint32_t key = valid ? keys_in[e] : 0u, id = valid ? ids_in[e] : 0u;
        const uint32_t d = (key >> shift) & 255u;
        unsigned long long same = __ballot(valid);  // the valid lanes with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        if (valid) {
            const uint32_t q = pos[d] + (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            if (q < n) {  // holds whenever hist is the histogram of keys_in
                keys_out[q] = key;
                ids_out[q] = id;
            }
        }
        __syncthreads();
        if (valid && lane == 63u - (uint32_t)__clzll(same)) pos[d] += (uint32_t)__popcll(same);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void dcn_det_rows_kernel(const uint32_t* __restrict__ keys, uint32_t* __restrict__ rows,
                                                           uint32_t n, uint32_t cells) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    if (k >= cells) return;
    if (i == 0 || keys[i - 1] != k) rows[2 * (size_t)k] = i;
    if (i == n - 1 || keys[i + 1] != k) rows[2 * (size_t)k + 1] = i + 1;
}

// The serial sum, from zero, of the entries ids[beg .. end) for channels c0 .. c0 + 3: w_q * (grad_col * mask), each product
// rounded (no contraction with the add), the corner weight and the mask recomputed from offset / mask.  `n`: the number of
// entries; the sorted ids are a permutation of 0 .. n-1, and the test keeps every read in bounds whatever the index holds.
__device__ __forceinline__ float4 det_sum(const BwdP& p, const uint32_t* __restrict__ ids, uint32_t n, uint32_t beg,
                                          uint32_t end, int c0) {
    const int C = p.C, HW = p.H * p.W;
    float4 acc = zero4();
    for (uint32_t i = beg; i < end; ++i) {
        const uint32_t id = ids[i];
        if (id >= n) continue;
        uint32_t pp;
        int tap, q;
        dcn_det_decode(id, &pp, &tap, &q);
        const int bi = (int)(pp / (uint32_t)HW), pix = (int)(pp - (uint32_t)bi * HW), b = p.b0 + bi;
        const int ho = pix / p.W, wo = pix - ho * p.W;
        const float oh = p.off[((size_t)b * 18 + 2 * tap) * HW + pix], ow = p.off[((size_t)b * 18 + 2 * tap + 1) * HW + pix];
        const float m = p.mask[((size_t)b * 9 + tap) * HW + pix];
        const float w = dcn_det_weight(dcn_det_sample_at(ho, wo, tap, oh, ow, p.H, p.W), q);
        const float4 g = ld4(p.gcol + (size_t)(id >> 2) * C + c0);
        acc.x += __fmul_rn(w, __fmul_rn(g.x, m));
        acc.y += __fmul_rn(w, __fmul_rn(g.y, m));
        acc.z += __fmul_rn(w, __fmul_rn(g.z, m));
        acc.w += __fmul_rn(w, __fmul_rn(g.w, m));
    }
    return acc;
}

// L lanes per cell (a power of two, 4 .. 64); lane l of the group owns channels 4l .. 4l + 3 of every block of 4L channels
__global__ __launch_bounds__(256) void dcn_det_gather_kernel(const BwdP p, const DetP d, int L) {
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    const uint32_t cell = gid / (uint32_t)L;
    const int l = (int)(gid - cell * (uint32_t)L);
    if (cell >= d.cells) return;
    const uint32_t beg = d.rows[2 * (size_t)cell], end = d.rows[2 * (size_t)cell + 1];
    const uint32_t stop = min(end, beg + (uint32_t)DCN_DET_CHUNK);
    float* out = p.gin + ((size_t)p.b0 * p.H * p.W + cell) * p.C;
    for (int c0 = 4 * l; c0 < p.C; c0 += 4 * L) *reinterpret_cast<float4*>(out + c0) = det_sum(p, d.ids, d.n, beg, stop, c0);
}

// Wave j looks at the sorted positions [j * CHUNK, (j + 1) * CHUNK).  Chunks of one list start CHUNK apart and a list's
// chunk t >= 1 starts at least CHUNK behind the list's begin, so at most one chunk t >= 1 starts in that range, and it
// belongs to the list that covers the range's first position.  Returns false where there is none.
__device__ __forceinline__ bool det_long_chunk(const DetP& d, uint32_t j, uint32_t* cell, uint32_t* beg, uint32_t* end,
                                               uint32_t* t) {
    const uint32_t pos = j * (uint32_t)DCN_DET_CHUNK;
    if (pos >= d.n) return false;
    const uint32_t k = d.keys[pos];
    if (k >= d.cells) return false;
    const uint32_t s0 = d.rows[2 * (size_t)k], e0 = d.rows[2 * (size_t)k + 1];
    if (s0 >= pos) return false;  // the list begins here: chunk 0 is the gather kernel's
    *t = (pos - s0 + (uint32_t)DCN_DET_CHUNK - 1u) / (uint32_t)DCN_DET_CHUNK;
    *beg = s0 + *t * (uint32_t)DCN_DET_CHUNK;
    *end = e0;
    *cell = k;
    return *beg < e0;
}

__global__ __launch_bounds__(256) void dcn_det_long_kernel(const BwdP p, const DetP d) {
    const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    uint32_t cell, beg, end, t;
    if (!det_long_chunk(d, j, &cell, &beg, &end, &t)) return;
    const uint32_t stop = min(end, beg + (uint32_t)DCN_DET_CHUNK);
    for (int c0 = 4 * lane; c0 < p.C; c0 += 256)
        *reinterpret_cast<float4*>(d.partial + (size_t)j * p.C + c0) = det_sum(p, d.ids, d.n, beg, stop, c0);
}

// the wave of a list's chunk 1 adds the list's partial rows to its line, chunks ascending
__global__ __launch_bounds__(256) void dcn_det_long_add_kernel(const BwdP p, const DetP d) {
    const uint32_t j = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    uint32_t cell, beg, end, t;
    if (!det_long_chunk(d, j, &cell, &beg, &end, &t) || t != 1u) return;
    float* out = p.gin + ((size_t)p.b0 * p.H * p.W + cell) * p.C;
    for (int c0 = 4 * lane; c0 < p.C; c0 += 256) {
        float4 acc = ld4(out + c0);
        for (uint32_t q = beg; q < end; q += (uint32_t)DCN_DET_CHUNK) {
            const float4 v = ld4(d.partial + (size_t)(q / (uint32_t)DCN_DET_CHUNK) * p.C + c0);
            acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
        }
        *reinterpret_cast<float4*>(out + c0) = acc;
    }
}

struct Plan {
    bool fast;
    int nb, nslab, slab_px;
    // f16x3 (dcn_bwd16.hip, conv_bwd16.hip): the weight gradient, grad_col; go_t's row length; the weight gradient's slabs
    bool wg16, dg16;
    int CoP;
    DcnWgrad16Plan w16;
};

Plan plan(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int dg, int precision) {
    Plan P;
    const int Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1, Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
    const size_t HWo = (size_t)Ho * Wo, TC = (size_t)C * kh * kw, Q = (size_t)B * HWo;
    P.fast = cp_dcn_backward_fast(C, kh, kw, sh, sw, ph, pw, dh, dw, dg);
    const size_t per_img = TC * HWo * 4;
    const size_t cap = (size_t)256 << 20;  // grad_col chunk: at most 256 MiB (or one image)
    P.nb = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, cap / per_img));
    const size_t tiles = ((TC + 31) / 32) * ((Co + 32 * WG_COUT - 1) / (32 * WG_COUT));
    size_t ns = (8192 + tiles - 1) / tiles;                                   // about 8 waves per SIMD
    ns = std::min(ns, std::max<size_t>(1, ((size_t)64 << 20) / (Co * TC * 4)));  // slabs: at most 64 MiB
    ns = std::max<size_t>(1, std::min(ns, (Q + 63) / 64));                    // at least 64 pixels a slab
    size_t spx = (Q + ns - 1) / ns;
    spx = (spx + 1) & ~(size_t)1;
    P.slab_px = (int)spx;
    P.nslab = (int)((Q + spx - 1) / spx);
    // f16x3: the fast geometry only; a chunk igemm16.hip cannot take as a 1x1 convolution's data gradient keeps gcol_kernel
    P.wg16 = P.fast && precision == CP_PREC_F16X3;
    P.CoP = P.wg16 ? (Co + 31) / 32 * 32 : Co;
    P.w16 = P.wg16 ? cp_dcn_wgrad16_plan((size_t)P.nb * HWo, C, P.CoP) : DcnWgrad16Plan{};
    P.dg16 = P.wg16 && cp_conv_dgrad16_s1_supported(P.nb, H, W, (int)TC, P.CoP, 1);
    return P;
}

// xh / gin (the NHWC copies of input and grad_input) exist on the fast path only
struct Ws {
    float *wt, *go_t, *xh, *gin, *gcol, *slab;
    // f16x3: the |max| slot block (slot 0: go_t, 1: x, 2: mask), the split copy of go_t, a chunk's split columns, the packed weight
    unsigned* slot;
    uint32_t *go16, *col16;
    void* wB;
};
Ws dcn_bwd_carve(Carve& c, const Plan& P, int B, int C, int H, int W, int Co, int Ho, int Wo, int T) {
    const size_t TC = (size_t)C * T, HWo = (size_t)Ho * Wo;
    Ws r;
    r.wt = c.take<float>((size_t)Co * TC * 4);
    r.go_t = c.take<float>((size_t)B * HWo * P.CoP * 4);
    r.xh = P.fast ? c.take<float>((size_t)B * H * W * C * 4) : nullptr;
    r.gin = P.fast ? c.take<float>((size_t)B * H * W * C * 4) : nullptr;
    r.gcol = c.take<float>((size_t)P.nb * TC * HWo * 4);
    // (f16x3: never less than the float32 plan's slabs, so that the mode's workspace is never the smaller one)
    const size_t slab32 = (size_t)P.nslab * Co * TC * 4;
    r.slab = c.take<float>(P.wg16 ? std::max(slab32, (size_t)P.w16.nslab * P.CoP * TC * 4) : slab32);
    r.slot = nullptr;
    r.go16 = r.col16 = nullptr;
    r.wB = nullptr;
    if (P.wg16) {  // (nothing is taken in float32: that workspace is the one it always was)
        r.slot = c.take<unsigned>(cp_amax_slot_bytes);
        r.go16 = c.take<uint32_t>((size_t)B * HWo * P.CoP * 4);
        r.col16 = c.take<uint32_t>((size_t)P.nb * TC * HWo * 4);
        r.wB = c.take<void>(P.dg16 ? cp_conv_dgrad16_pack_bytes((int)TC, P.CoP, 1, 1) : 0);
    }
    return r;
}

// the deterministic path's index of one chunk: keys and ids double-buffered for the radix passes (16 bytes an entry), the
// digit table, the lists' bounds and the long lists' partial rows
struct DetWs {
    uint32_t *keys[2], *ids[2], *hist, *sums, *rows;
    float* partial;
};
DetWs dcn_det_carve(Carve& c, const Plan& P, int C, int H, int W) {
    const size_t cells = (size_t)P.nb * H * W, n = cells * 36;
    DetWs r;
    for (int i = 0; i < 2; ++i) r.keys[i] = c.take<uint32_t>(n * 4);
    for (int i = 0; i < 2; ++i) r.ids[i] = c.take<uint32_t>(n * 4);
    const size_t m = 256 * ((n + RS_TILE - 1) / RS_TILE);
    r.hist = c.take<uint32_t>(m * 4);
    r.sums = c.take<uint32_t>((m + SCAN_SEG - 1) / SCAN_SEG * 4);
    r.rows = c.take<uint32_t>(cells * 2 * 4);
    r.partial = c.take<float>(((n + DCN_DET_CHUNK - 1) / DCN_DET_CHUNK) * C * 4);
    return r;
}

}  // namespace

bool cp_dcn_backward_fast(int C, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int dg) {
    return kh == 3 && kw == 3 && sh == 1 && sw == 1 && ph == 1 && pw == 1 && dh == 1 && dw == 1 && dg == 1 && C % 16 == 0;
}

size_t cp_dcn_backward_ws_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                                int dw, int dg, int precision) {
    const int Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1, Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
    Carve c{nullptr};
    dcn_bwd_carve(c, plan(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg, precision), B, C, H, W, Co, Ho, Wo, kh * kw);
    return c.off;
}

int cp_dcn_backward_prec_mask(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                              int dg, int precision) {
    const Plan P = plan(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg, precision);
    return (P.wg16 ? 1 : 0) | (P.dg16 ? 2 : 0);
}

namespace {

BwdP bwd_params(const DcnBwdArgs& a, const Plan& P, const Ws& r) {
    BwdP p;
    p.x = a.input;
    p.xh = r.xh;
    p.wt = r.wt;
    p.off = a.offset;
    p.mask = a.mask;
    p.go = a.grad_output;
    p.go_t = r.go_t;
    p.gcol = r.gcol;
    p.gin = P.fast ? r.gin : a.grad_input;
    p.goff = a.grad_offset;
    p.gmask = a.grad_mask;
    p.slab = r.slab;
    p.B = a.B, p.C = a.C, p.H = a.H, p.W = a.W, p.Co = a.Co, p.Ho = a.Ho, p.Wo = a.Wo;
    p.kh = a.kh, p.kw = a.kw, p.sh = a.sh, p.sw = a.sw, p.ph = a.ph, p.pw = a.pw, p.dh = a.dh, p.dw = a.dw, p.dg = a.dg;
    p.b0 = 0, p.nb = P.nb, p.slab_px = P.slab_px, p.nslab = P.nslab;
    return p;
}

// step 1: wt, go_t, and on the fast path x staged NHWC.  f16x3 (step 1'): go_t padded with its |max|, the |max| of x and of the
// mask, the split copy of go_t and the packed weight.
int stage(hipStream_t s, const DcnBwdArgs& a, const Plan& P, const Ws& r) {
    const int T = a.kh * a.kw, HWo = a.Ho * a.Wo;
    hipLaunchKernelGGL(wt_kernel, dim3(256), dim3(256), 0, s, a.weight, r.wt, a.Co, a.C, T);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    int rc;
    if (P.wg16) {
        if (hipMemsetAsync(r.slot, 0, cp_amax_slot_bytes, s) != hipSuccess) return CP_ERR_LAUNCH;
        rc = cp_launch_dcn_go_pad(s, a.grad_output, r.go_t, a.B, a.Co, P.CoP, HWo, r.slot);
    } else {
        rc = cp_launch_nchw_to_nhwc(a.grad_output, r.go_t, a.B, a.Co, a.Ho, a.Wo, a.Co, s);
    }
    if (rc != CP_OK) return rc;
    if (P.fast) {
        rc = cp_launch_nchw_to_nhwc(a.input, r.xh, a.B, a.C, a.H, a.W, a.C, s);
        if (rc != CP_OK) return rc;
    }
    if (!P.wg16) return CP_OK;
    rc = cp_launch_absmax32(a.input, (size_t)a.B * a.C * a.H * a.W, r.slot + 1, s);
    if (rc == CP_OK) rc = cp_launch_absmax32(a.mask, (size_t)a.B * 9 * HWo, r.slot + 2, s);
    if (rc == CP_OK) rc = cp_launch_split16(r.go_t, r.go16, (size_t)a.B * HWo * P.CoP, r.slot, s);
    if (rc == CP_OK && P.dg16) rc = cp_launch_conv_dgrad16_pack(s, r.wt, r.wB, 9 * a.C, a.Co, P.CoP, 1, 1);
    return rc;
}

// f16x3, per chunk (p.b0, p.nb): grad_col pixel-major, the chunk's split columns and their sums into the slabs
int chunk16(hipStream_t s, const DcnBwdArgs& a, const Plan& P, const Ws& r, const BwdP& p) {
    const int TC = 9 * a.C, HW = a.H * a.W;
    const float* go_t = r.go_t + (size_t)p.b0 * HW * P.CoP;
    if (P.dg16) {
        // the 1x1 convolution 9C -> Co on the chunk's pixels: its data gradient from gs = go_t, w = wt [Co][9C][1]
        const ConvBwdArgs ca{nullptr, nullptr, nullptr, nullptr, r.gcol, nullptr, nullptr, p.nb, a.H, a.W, TC, a.Co, 1, 1, 1, 0};
        const int rc = cp_launch_conv_dgrad16_s1(s, ca, go_t, P.CoP, r.wB, nullptr, r.slot);
        if (rc != CP_OK) return rc;
    } else {
        hipLaunchKernelGGL(gcol_kernel<true>, dim3((HW + 127) / 128, (TC + 127) / 128, p.nb), dim3(256), 0, s, p);
        if (!launch_ok()) return CP_ERR_LAUNCH;
    }
    int rc = cp_launch_dcn_col16(s, r.xh, a.offset, a.mask, r.col16, r.slot + 1, r.slot + 2, p.b0, p.nb, a.C, a.H, a.W);
    if (rc != CP_OK) return rc;
    return cp_launch_dcn_wgrad16_slabs(s, r.go16 + (size_t)p.b0 * HW * P.CoP, r.col16, r.slab, p.nb * HW, a.C, P.CoP, P.w16, p.b0 > 0);
}

// step 3 (p.b0 = 0, p.nb = P.nb): grad_weight from the slabs -- f16x3: the chunks have filled them -- and grad_bias
int weight_bias(hipStream_t s, const DcnBwdArgs& a, const Plan& P, const Ws& r, const BwdP& p) {
    const int T = a.kh * a.kw, TC = a.C * T;
    if (P.wg16) {
        const int rc = cp_launch_dcn_wgrad16_reduce(s, r.slab, a.grad_weight, P.w16.nslab, a.Co, P.CoP, a.C, r.slot, r.slot + 1, r.slot + 2);
        if (rc != CP_OK) return rc;
    } else {
        const dim3 wg_grid((TC + 127) / 128, 1, P.nslab);
        if (a.Co <= 32)
            hipLaunchKernelGGL(wgrad_kernel<1>, wg_grid, dim3(256), 0, s, p);
        else if (a.Co <= 64)
            hipLaunchKernelGGL(wgrad_kernel<2>, wg_grid, dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL(wgrad_kernel<WG_COUT>, dim3(wg_grid.x, (a.Co + 32 * WG_COUT - 1) / (32 * WG_COUT), P.nslab),
                               dim3(256), 0, s, p);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(1024), dim3(256), 0, s, (const float*)p.slab, a.grad_weight, P.nslab, a.Co,
                           a.C, T);
        if (!launch_ok()) return CP_ERR_LAUNCH;
    }
    return cp_launch_rowsum_nchw(a.grad_output, a.grad_bias, a.B, a.Co, a.Ho * a.Wo, s);
}

}  // namespace

int cp_launch_dcn_backward(hipStream_t s, const DcnBwdArgs& a, void* ws, int precision) {
    const Plan P = plan(a.B, a.C, a.H, a.W, a.Co, a.kh, a.kw, a.sh, a.sw, a.ph, a.pw, a.dh, a.dw, a.dg, precision);
    const int T = a.kh * a.kw, TC = a.C * T;
    Carve cv{(char*)ws};
    const Ws r = dcn_bwd_carve(cv, P, a.B, a.C, a.H, a.W, a.Co, a.Ho, a.Wo, T);
    BwdP p = bwd_params(a, P, r);
    const int HWo = a.Ho * a.Wo;
    const size_t in_bytes = (size_t)a.B * a.C * a.H * a.W * 4;

    int rc = stage(s, a, P, r);
    if (rc != CP_OK) return rc;
    if (hipMemsetAsync(p.gin, 0, in_bytes, s) != hipSuccess) return CP_ERR_LAUNCH;

    for (int b0 = 0; b0 < a.B; b0 += P.nb) {
        p.b0 = b0;
        p.nb = std::min(P.nb, a.B - b0);
        if (P.wg16) {
            rc = chunk16(s, a, P, r, p);
            if (rc != CP_OK) return rc;
        } else {
            hipLaunchKernelGGL(gcol_kernel<false>, dim3((HWo + 127) / 128, (TC + 127) / 128, p.nb), dim3(256), 0, s, p);
            if (!launch_ok()) return CP_ERR_LAUNCH;
        }
        if (P.fast) {
            const dim3 grid((a.Wo + PT_X - 1) / PT_X, (a.Ho + PT_Y - 1) / PT_Y, p.nb);
            if (a.C % 32 == 0 && P.wg16)
                hipLaunchKernelGGL((dcn_bwd_halo_kernel<32, true>), grid, dim3(576), 0, s, p);
            else if (P.wg16)
                hipLaunchKernelGGL((dcn_bwd_halo_kernel<16, true>), grid, dim3(576), 0, s, p);
            else if (a.C % 32 == 0)
                hipLaunchKernelGGL((dcn_bwd_halo_kernel<32, false>), grid, dim3(576), 0, s, p);
            else
                hipLaunchKernelGGL((dcn_bwd_halo_kernel<16, false>), grid, dim3(576), 0, s, p);
        } else {
            const size_t n = (size_t)p.nb * a.dg * T * HWo;
            const size_t blocks = std::min<size_t>((n + 255) / 256, 65536);
            hipLaunchKernelGGL(dcn_bwd_generic_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p);
        }
        if (!launch_ok()) return CP_ERR_LAUNCH;
    }
    p.b0 = 0;
    p.nb = P.nb;
    rc = weight_bias(s, a, P, r, p);
    if (rc != CP_OK) return rc;
    if (P.fast) return cp_launch_nhwc_to_nchw(p.gin, a.grad_input, a.B, a.C, a.H, a.W, a.C, s);
    return CP_OK;
}

size_t cp_dcn_backward_det_ws_bytes(int B, int C, int H, int W, int Co, int precision) {
    Carve c{nullptr};
    const Plan P = plan(B, C, H, W, Co, 3, 3, 1, 1, 1, 1, 1, 1, 1, precision);
    dcn_bwd_carve(c, P, B, C, H, W, Co, H, W, 9);
    dcn_det_carve(c, P, C, H, W);
    return c.off;
}

// The launch sequence of cp_launch_dcn_backward on the fast geometry with the data kernel replaced: pixel-major grad_col,
// the coord kernel, the index, its sort and the gather; no memset of the input gradient (the gather stores every line).
int cp_launch_dcn_backward_det(hipStream_t s, const DcnBwdArgs& a, void* ws, int precision) {
    const Plan P = plan(a.B, a.C, a.H, a.W, a.Co, 3, 3, 1, 1, 1, 1, 1, 1, 1, precision);
    const int T = 9, TC = a.C * T, HW = a.H * a.W;
    Carve cv{(char*)ws};
    const Ws r = dcn_bwd_carve(cv, P, a.B, a.C, a.H, a.W, a.Co, a.Ho, a.Wo, T);
    const DetWs dw = dcn_det_carve(cv, P, a.C, a.H, a.W);
    BwdP p = bwd_params(a, P, r);

    int rc = stage(s, a, P, r);
    if (rc != CP_OK) return rc;

    int L = 4;  // lanes per destination cell: the power of two that covers C / 4 float4 pieces, 64 at most
    while (L < 64 && 4 * L < a.C) L *= 2;
    for (int b0 = 0; b0 < a.B; b0 += P.nb) {
        p.b0 = b0;
        p.nb = std::min(P.nb, a.B - b0);
        const uint32_t cells = (uint32_t)p.nb * HW, n = cells * 36u, ntiles = (n + RS_TILE - 1) / RS_TILE;
        const unsigned tap_blocks = (cells * 9u + 255u) / 256u;
        if (P.wg16) {
            rc = chunk16(s, a, P, r, p);
            if (rc != CP_OK) return rc;
        } else {
            hipLaunchKernelGGL(gcol_kernel<true>, dim3((HW + 127) / 128, (TC + 127) / 128, p.nb), dim3(256), 0, s, p);
            if (!launch_ok()) return CP_ERR_LAUNCH;
        }
        hipLaunchKernelGGL(dcn_det_coord_kernel, dim3(tap_blocks), dim3(256), 0, s, p);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        hipLaunchKernelGGL(dcn_det_index_kernel, dim3(tap_blocks), dim3(256), 0, s, p, dw.keys[0], dw.ids[0], cells);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        int src = 0;
        for (int pass = 0; pass < dcn_det_passes(cells); ++pass, src ^= 1) {
            hipLaunchKernelGGL(rs_hist_kernel, dim3(ntiles), dim3(256), 0, s, dw.keys[src], dw.hist, n, 8 * pass, ntiles);
            if (!launch_ok()) return CP_ERR_LAUNCH;
            const uint32_t m = 256u * ntiles, segs = (m + SCAN_SEG - 1) / SCAN_SEG;
            hipLaunchKernelGGL(rs_scan_sums_kernel, dim3(segs), dim3(256), 0, s, dw.hist, dw.sums, m);
            if (!launch_ok()) return CP_ERR_LAUNCH;
            hipLaunchKernelGGL(rs_scan_apply_kernel, dim3(segs), dim3(256), 0, s, dw.hist, dw.sums, m);
            if (!launch_ok()) return CP_ERR_LAUNCH;
            hipLaunchKernelGGL(rs_scatter_kernel, dim3(ntiles), dim3(64), 0, s, dw.keys[src], dw.ids[src], dw.keys[src ^ 1],
                               dw.ids[src ^ 1], dw.hist, n, 8 * pass, ntiles);
            if (!launch_ok()) return CP_ERR_LAUNCH;
        }
        const DetP d{dw.keys[src], dw.ids[src], dw.rows, dw.partial, n, cells};
        if (hipMemsetAsync(dw.rows, 0, (size_t)cells * 8, s) != hipSuccess) return CP_ERR_LAUNCH;
        hipLaunchKernelGGL(dcn_det_rows_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, d.keys, d.rows, n, cells);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        hipLaunchKernelGGL(dcn_det_gather_kernel, dim3((cells * (uint32_t)L + 255u) / 256u), dim3(256), 0, s, p, d, L);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        const unsigned long_blocks = ((n + DCN_DET_CHUNK - 1) / DCN_DET_CHUNK + 3u) / 4u;
        hipLaunchKernelGGL(dcn_det_long_kernel, dim3(long_blocks), dim3(256), 0, s, p, d);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        hipLaunchKernelGGL(dcn_det_long_add_kernel, dim3(long_blocks), dim3(256), 0, s, p, d);
        if (!launch_ok()) return CP_ERR_LAUNCH;
    }
    p.b0 = 0;
    p.nb = P.nb;
    rc = weight_bias(s, a, P, r, p);
    if (rc != CP_OK) return rc;
    return cp_launch_nhwc_to_nchw(p.gin, a.grad_input, a.B, a.C, a.H, a.W, a.C, s);
}
