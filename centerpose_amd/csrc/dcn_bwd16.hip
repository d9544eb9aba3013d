// The f16x3 form of the DCNv2 backward's weight gradient (cp_dcnv2_backward_prec with CP_PREC_F16X3; fast geometry: 3x3, stride 1,
// pad 1, dilation 1, one deformable group, C % 16 == 0).  dcn_bwd.hip's wgrad_kernel rebuilds every modulated-im2col value in the
// lane that feeds it to the matrix core, once per Co tile group: four scalar loads per K = 2 step.  Here the columns of a chunk of
// images are materialised once, as whole lines, and the weight gradient is the one of a 1x1 convolution with 9C input channels
// over them: conv_bwd16.hip's split-binary16 arithmetic (hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16, float32 accumulation,
// exact power-of-two pre-scales) and its slab kernel's loop shape.  grad_col, the other contraction, is that convolution's
// stride-1 data gradient and runs on conv_bwd16.hip's kernels unchanged (dcn_bwd.hip launches it).
//
//   dcn_go_pad_kernel    go_t [pixel][CoP]: grad_output transposed, zero-padded to 32 channels, with its |max| (both contractions'
//                        A operand: float32 for the data gradient's loader, split by cp_launch_split16 for the weight gradient)
//   dcn_col16_kernel     col16[image][pixel][tap][C], pixel-major (gcol_kernel<true>'s layout): lanes run along C, four channels
//                        each, so the four corner loads are float4 pieces of one NHWC line and the store is one 16-byte piece
//                        of a contiguous run.  The value is wgrad_kernel's float32 expression (make_sample, the same blend order,
//                        times the mask, zero outside (-1, H) x (-1, W)), times 2^e, stored as a split dword (split_kernel's form).
//                        Range.  2^e comes from the bound  A = |max x| * |max mask|  (two |max| slots, one pass each over x and
//                        the mask: the columns are never read twice).  |blend| <= (w1 + w2 + w3 + w4) |max x| with rounded
//                        weights whose sum is at most 1 + 4 * 2^-24, three rounded adds and one rounded product with the mask:
//                        |col| <= A (1 + 2^-20).  cp_amax_to_scale puts A * 2^e into [2^14, 2^15), so |col * 2^e| < 2^15 (1 + 2^-20),
//                        a factor two below binary16's largest number -- for ANY mask, not only a sigmoid's output, because the
//                        mask's own |max| is in the bound.  Where A itself overflows float32 the float32 mode's column does as
//                        well; where it underflows the scale is the clamped 2^125 and nothing can overflow.
//   dcn_wgrad16_kernel   slab[s][co][k] (+)= sum over the pixels q of slab s of go16[q][co] * col16[q][k]: wgrad16_kernel's jobs
//                        (a wave: NH 32-row co tiles x 2 32-column k tiles), fragments (a lane owns one channel, lane & 31, and
//                        eight consecutive pixels, lane >> 5 selects which eight: every load is a whole 128-byte line per
//                        half-wave) and pipeline (two fragment sets, the loop unrolled by two, the step after the one in the
//                        matrix core always in flight, no branch between the loads: the ragged end of a slab and the ragged last
//                        k tile -- 9C is a multiple of 16, not of 32 -- are zeros of out-of-range buffer loads; with selects on
//                        clamped addresses the compiler sank every load into a branch of its own and waited for each).  Pixels are
//                        one flat sequence, so there are no row ends.  `accum`: a later chunk of images adds its sums to the slabs
//                        of the first (chunks in order on one stream: the order is fixed).
//   dcn_wgrad16_reduce_kernel  grad_weight[co][c][tap] = (two_level_sum of the slabs) * 2^-e_g * 2^-e_col, exact multiplies; the
//                        permutation to [Co][C][kh][kw] stays here.
// No atomics but the |max| slots'; every sum has a fixed order.
#include "op_common.h"
#include "igemm16_common.h"
#include "dcn_bwd_sample.h"

#include <algorithm>

namespace {

// (2^e, 2^-e) of the columns: from the bound |max x| * |max mask|
__device__ __forceinline__ void col_scale(const unsigned* x_amax, const unsigned* m_amax, float* fwd, float* inv) {
    const float bound = __uint_as_float(cp_amax_read(x_amax)) * __uint_as_float(cp_amax_read(m_amax));
    cp_amax_to_scale(__float_as_uint(bound), fwd, inv);
}

// item e (grid-stride): sample e / (C / 4) = (image of the chunk, pixel, tap), channels 4 (e % (C / 4)) .. + 3; n = nb H W 9 C / 4 items
__global__ __launch_bounds__(256) void dcn_col16_kernel(const float* __restrict__ xh, const float* __restrict__ off,
                                                        const float* __restrict__ mask, uint32_t* __restrict__ col16,
                                                        const unsigned* __restrict__ x_amax, const unsigned* __restrict__ m_amax, int b0,
                                                        int C, int H, int W, size_t n) {
    const int c4 = C >> 2, HW = H * W;
    float fwd, inv;
    col_scale(x_amax, m_amax, &fwd, &inv);
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const size_t smp = e / c4;
        const int c = (int)(e - smp * c4) * 4;
        const size_t pp = smp / 9;
        const int tap = (int)(smp - pp * 9);
        const int bi = (int)(pp / HW), pix = (int)(pp - (size_t)bi * HW), b = b0 + bi;
        const int ho = pix / W, wo = pix - ho * W;
        const int i = tap / 3, j = tap - 3 * i;
        const float oh = off[((size_t)b * 18 + 2 * tap) * HW + pix], ow = off[((size_t)b * 18 + 2 * tap + 1) * HW + pix];
        const float m = mask[((size_t)b * 9 + tap) * HW + pix];
        const Sample s = make_sample((float)(ho - 1 + i) + oh, (float)(wo - 1 + j) + ow, H, W);
        const float* xb = xh + (size_t)b * HW * C + c;
        const float4 v1 = s.c1 ? ld4(xb + ((size_t)s.y0 * W + s.x0) * C) : zero4();
        const float4 v2 = s.c2 ? ld4(xb + ((size_t)s.y0 * W + s.x0 + 1) * C) : zero4();
        const float4 v3 = s.c3 ? ld4(xb + ((size_t)(s.y0 + 1) * W + s.x0) * C) : zero4();
        const float4 v4 = s.c4 ? ld4(xb + ((size_t)(s.y0 + 1) * W + s.x0 + 1) * C) : zero4();
        const float a1[4] = {v1.x, v1.y, v1.z, v1.w}, a2[4] = {v2.x, v2.y, v2.z, v2.w};
        const float a3[4] = {v3.x, v3.y, v3.z, v3.w}, a4[4] = {v4.x, v4.y, v4.z, v4.w};
        u32x4 o;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            // the forward's column value: (w1 v1 + w2 v2 + w3 v3 + w4 v4) * mask, zero outside (-1, H) x (-1, W)
            const float val = (s.hh * s.hw) * a1[u] + (s.hh * s.lw) * a2[u] + (s.lh * s.hw) * a3[u] + (s.lh * s.lw) * a4[u];
            const float bv = s.in ? val * m : 0.f;
            o[u] = split_dword(bv * fwd);
        }
        *reinterpret_cast<u32x4*>(col16 + e * 4) = o;
    }
}

// grad_output [B,Co,HW] -> go_t [B HW][CoP] float32, zeros in the pad lanes Co .. CoP - 1 (CoP % 32 == 0), through a 32 x 32 LDS tile
// (ewise.hip's tiled transposition), and its |max| into `slot`
__global__ __launch_bounds__(256) void dcn_go_pad_kernel(const float* __restrict__ in, float* __restrict__ out, int Co, int CoP, int HW,
                                                         unsigned* __restrict__ slot) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 256 threads: 8 rows per pass
    float m = 0.f;
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, p = p0 + tx;
        const float v = (c < Co && p < HW) ? in[((size_t)b * Co + c) * HW + p] : 0.f;
        tile[r][tx] = v;
        m = fmaxf(m, fabsf(v));
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int p = p0 + r, c = c0 + tx;
        if (p < HW) out[((size_t)b * HW + p) * CoP + c] = tile[tx][r];
    }
    cp_amax_commit(slot, m);
}

template <int NH>
struct DFrag {
    uint32_t a[NH][8], b[2][8];
};

// go16 [Q][CoP] and col16 [Q][TC] from the chunk's first pixel; slab s owns the pixels [s slab_px, (s + 1) slab_px) of Q
template <int NH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void dcn_wgrad16_kernel(
    const uint32_t* __restrict__ go16, const uint32_t* __restrict__ col16, float* __restrict__ slab, int Q, int CoP, int TC, int slab_px,
    int accum) {
    const int KT = (TC + 31) / 32, KJ = (KT + 1) / 2;
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int job = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int hg = job / KJ, kj = job - hg * KJ;
    if (hg * 32 * NH >= CoP) return;
    const int q_beg = blockIdx.z * slab_px, q_end = min(Q, q_beg + slab_px);
    if (q_beg >= Q) return;  // (a partial last chunk has fewer slabs; wave-uniform)
    const int h0 = hg * 32 * NH;
    // Both operands through buffer descriptors that cover exactly the slab's pixels (igemm16_common.h's idiom): a load past the
    // slab's end, or from a masked lane's offset, returns zero without a branch or a select around it.  The whole offset is in
    // the lane's register: the range check does not see a scalar offset.
    const unsigned qn = (unsigned)(q_end - q_beg);
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(go16 + (size_t)q_beg * CoP, qn * (unsigned)CoP * 4u);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(col16 + (size_t)q_beg * TC, qn * (unsigned)TC * 4u);
    unsigned va[NH], vb[2];  // byte offsets of the lane's element in pixel 8 (lane >> 5) of a step
    bool kv[2];              // the lane's column of k tile n exists (the last tile of 9C = 16 (mod 32) columns is half empty)
#pragma unroll
    for (int t = 0; t < NH; ++t) va[t] = (unsigned)(8 * hh * CoP + h0 + 32 * t + r) * 4u;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int k = (kj * 2 + n) * 32 + r;
        kv[n] = k < TC;
        vb[n] = kv[n] ? (unsigned)(8 * hh * TC + k) * 4u : 0x80000000u;  // (stays out of range whatever is added below)
    }
    f32x16 acc[NH][2];
#pragma unroll
    for (int t = 0; t < NH; ++t)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][n][e] = 0.f;
    unsigned sa = 0, sb = 0;  // byte offsets of the next step to request (wave-uniform)
    auto load = [&](DFrag<NH>& f) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int t = 0; t < NH; ++t) f.a[t][j] = __builtin_amdgcn_raw_buffer_load_b32(ra, (int)(va[t] + sa + (unsigned)(j * CoP) * 4u), 0, 0);
#pragma unroll
            for (int n = 0; n < 2; ++n) f.b[n][j] = __builtin_amdgcn_raw_buffer_load_b32(rb, (int)(vb[n] + sb + (unsigned)(j * TC) * 4u), 0, 0);
        }
        sa += 16u * (unsigned)CoP * 4u;
        sb += 16u * (unsigned)TC * 4u;
    };
    auto mma = [&](const DFrag<NH>& f) {
        h8 ah[NH], al[NH], bh[2], bl[2];
#pragma unroll
        for (int t = 0; t < NH; ++t) unpack8(f.a[t], ah[t], al[t]);
#pragma unroll
        for (int n = 0; n < 2; ++n) unpack8(f.b[n], bh[n], bl[n]);
#pragma unroll
        for (int t = 0; t < NH; ++t)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[t][n] = mma3(ah[t], al[t], bh[n], bl[n], acc[t][n]);
    };
    const int total = (q_end - q_beg + 15) / 16;
    DFrag<NH> f0, f1;
    load(f0);
    for (int it = 0; it < total; it += 2) {
        load(f1);
        mma(f0);
        load(f0);
        mma(f1);  // (an odd count's last step: zeros)
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
                float* dst = out + (size_t)h * TC + k;
                *dst = accum ? *dst + acc[t][n][e] : acc[t][n][e];
            }
        }
}

// conv_bwd.hip's wgrad_reduce_kernel for these slabs [co][tap * C + c] (co < Co of CoP rows): threads walk the slabs' own element
// order and scatter the one write; the finished sum is multiplied by 2^-e_g, then 2^-e_col
__global__ __launch_bounds__(256) void dcn_wgrad16_reduce_kernel(const float* __restrict__ slab, float* __restrict__ gw, int nslab, int Co,
                                                                 int CoP, int C, const unsigned* __restrict__ g_amax,
                                                                 const unsigned* __restrict__ x_amax, const unsigned* __restrict__ m_amax) {
    __shared__ float red[256];
    float fw, gi, ci;
    cp_amax_to_scale(cp_amax_read(g_amax), &fw, &gi);
    col_scale(x_amax, m_amax, &fw, &ci);
    const size_t TC = (size_t)9 * C, n = (size_t)Co * TC, ss = (size_t)CoP * TC;
    for (size_t base = (size_t)blockIdx.x * 32; base < n; base += (size_t)gridDim.x * 32) {  // (uniform per workgroup)
        const size_t i = base + (threadIdx.x & 31);
        float t = two_level_sum(red, i < n, nslab, 0.f, [&](float v, int s) { return v + slab[(size_t)s * ss + i]; });
        t = cp_scale_pow2(t, gi, ci);
        if (threadIdx.x < 32 && i < n) {
            const size_t h = i / TC;
            const int k = (int)(i - h * TC), tap = k / C, c = k - tap * C;
            gw[(h * C + c) * 9 + tap] = t;
        }
        __syncthreads();
    }
}

}  // namespace

// about two waves per SIMD and at most 512 slabs (cp_conv_wgrad_plan's rule), at least 256 pixels a slab, at most 64 MiB of slabs
DcnWgrad16Plan cp_dcn_wgrad16_plan(size_t Q, int C, int CoP) {
    DcnWgrad16Plan P;
    const size_t TC = (size_t)9 * C;
    P.nh = CoP % 64 == 0 ? 2 : 1;
    const int KT = (int)((TC + 31) / 32);
    P.jobs = (CoP / (32 * P.nh)) * ((KT + 1) / 2);
    size_t ns = std::min<size_t>(512, (2048 + P.jobs - 1) / P.jobs);
    ns = std::min(ns, std::max<size_t>(1, ((size_t)64 << 20) / ((size_t)CoP * TC * 4)));
    ns = std::max<size_t>(1, std::min(ns, (Q + 255) / 256));
    // (a slab's rows of either operand stay below 2^30 bytes: the kernel addresses them with 32-bit offsets)
    ns = std::max(ns, (Q * std::max<size_t>(CoP, TC) * 4 + ((size_t)1 << 30) - 1) >> 30);
    size_t spx = (Q + ns - 1) / ns;
    spx = (spx + 15) & ~(size_t)15;
    P.slab_px = (int)spx;
    P.nslab = (int)((Q + spx - 1) / spx);
    return P;
}

int cp_launch_dcn_go_pad(hipStream_t s, const float* go, float* go_t, int B, int Co, int CoP, int HW, unsigned* slot) {
    hipLaunchKernelGGL(dcn_go_pad_kernel, dim3((HW + 31) / 32, CoP / 32, B), dim3(256), 0, s, go, go_t, Co, CoP, HW, slot);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_dcn_col16(hipStream_t s, const float* xh, const float* off, const float* mask, uint32_t* col16, const unsigned* x_amax,
                        const unsigned* m_amax, int b0, int nb, int C, int H, int W) {
    const size_t n = (size_t)nb * H * W * 9 * (C / 4);
    hipLaunchKernelGGL(dcn_col16_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 16384)), dim3(256), 0, s, xh, off, mask, col16, x_amax, m_amax, b0, C,
                       H, W, n);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_dcn_wgrad16_slabs(hipStream_t s, const uint32_t* go16, const uint32_t* col16, float* slab, int Q, int C, int CoP,
                                const DcnWgrad16Plan& P, int accum) {
    const dim3 wg((P.jobs + 3) / 4, 1, P.nslab);
    if (P.nh == 2)
        hipLaunchKernelGGL(dcn_wgrad16_kernel<2>, wg, dim3(256), 0, s, go16, col16, slab, Q, CoP, 9 * C, P.slab_px, accum);
    else
        hipLaunchKernelGGL(dcn_wgrad16_kernel<1>, wg, dim3(256), 0, s, go16, col16, slab, Q, CoP, 9 * C, P.slab_px, accum);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_dcn_wgrad16_reduce(hipStream_t s, const float* slab, float* gw, int nslab, int Co, int CoP, int C, const unsigned* g_amax,
                                 const unsigned* x_amax, const unsigned* m_amax) {
    const size_t rg = std::min<size_t>(((size_t)Co * 9 * C + 31) / 32, 8192);
    hipLaunchKernelGGL(dcn_wgrad16_reduce_kernel, dim3((unsigned)rg), dim3(256), 0, s, slab, gw, nslab, Co, CoP, C, g_amax, x_amax, m_amax);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
