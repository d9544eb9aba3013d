// Backward of the two transposed convolutions of the up-sampling paths (cp_conv_transpose2d_backward_nhwc / _prec_nhwc), float32
// NHWC, no atomics (but the f16x3 mode's |max| slots'), every sum in a fixed order:
//   depth-wise  IDAUp's `up` (pose_dla_dcn.py:402-417): ConvTranspose2d(C, C, k = 2f, stride f, padding f/2, groups C), the
//               forward of upsample_add_kernel (ewise.hip) in upadd_common.h's notation.  New kernels, below.
//   dense       resnet_dcn.py:232-240's deconv layers: ConvTranspose2d(Cin, Cout, 4, stride 2, padding 1).  No kernel of its own:
//               the transposed convolution is the adjoint of conv2d(., w, stride 2, pad 1) with w [Cin,Cout,4,4] read as
//               [out,in,4,4], so its data gradient IS that convolution of grad_out (the exact-f32 implicit GEMM of igemm.hip) and
//               its weight gradient is that convolution's weight gradient with the roles of input and output gradient swapped
//               (cp_launch_conv_wgrad: `x` = grad_out, `gs` = x; wgrad_reduce_kernel then writes [Cin][Cout][4][4]).
//               CP_PREC_F16X3 runs the same two contractions in split binary16 on what conv_bwd16.hip and igemm16.hip
//               provide: wgrad16_kernel on the split copies of grad_out and x, and cp_launch_conv16 on w packed as a forward
//               convolution's weight (cp_pack_f16x3).  The depth-wise kernels have no matrix product: float32 in either mode.
#include "op_common.h"

#include <algorithm>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

namespace {

// Depth-wise backward, both gradients from one pass over grad_out:
//   grad_x[b,iy,ix,c] = sum_{ky,kx} go[b, iy f - p + ky, ix f - p + kx, c] * w[c,ky,kx]
//   grad_w[c,ky,kx]   = sum_{b,iy,ix} x[b,iy,ix,c] * go[b, iy f - p + ky, ix f - p + kx, c]
// A thread owns one source pixel, one channel quad (16 bytes) and one group of 4 x 4 taps: k = 4 has one group (G = 1), k = 8
// four (G = 4, one per wave-sized quarter of the workgroup).  It requests its sixteen grad_out pieces -- and x -- before using
// any, without a branch: a tap outside the grid (and a pixel beyond the slab) is requested beyond the buffer descriptor and
// comes back as zeros.  Each piece feeds both sums while it is in registers, so grad_out is not read once per gradient; the
// windows of neighbouring source pixels overlap (a piece is wanted by 2 x 2 of them), which the caches absorb: those threads
// sit in the same or the neighbouring workgroup.  Lanes of one pixel are consecutive channel quads, so a request covers whole
// 128-byte lines wherever C % 32 == 0.
//   grad_x: the group's sixteen products in (ky, kx) order from 0; with G = 4 the groups' sums then meet in LDS and are added
//           in group order.  Not computed and not stored when gx is NULL.
//   grad_w: sixteen float4 accumulators per thread over the pixels of its pixel lane, ascending; at the end the pixel lanes
//           are added in lane order through LDS and the workgroup writes part[slab][tap][C].  dw_wgrad_reduce_kernel adds the
//           slabs by two_level_sum.
// LDS: [256 float4 exchange][k k C weights as [tap][channel], one ds_read_b128 per lane and tap].
template <int G>
__global__ __launch_bounds__(256) void dw_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ go, float* __restrict__ gx,
                                                     float* __restrict__ part, int B, int H, int W, int C, int f, int px_per_slab) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4* xch = reinterpret_cast<float4*>(smem);
    float* wt = smem + 1024;
    const int k = 2 * f, kk = k * k, p = f / 2, C4 = C >> 2;
    for (int i = threadIdx.x; i < C * kk; i += 256) {
        const int c = i / kk, t = i - c * kk;
        wt[t * C + c] = w[i];
    }
    __syncthreads();
    constexpr int IT = 256 / G;  // (pixel lane, channel quad) items per tap group
    const int tg = threadIdx.x / IT, local = threadIdx.x - tg * IT;
    const int PL = IT / C4;  // >= 1: C4 <= IT is part of the accepted geometry
    const int pl = local / C4, cq = local - pl * C4;
    const bool lane_on = pl < PL;
    const int ty0 = (tg / (k / 4)) * 4, tx0 = (tg % (k / 4)) * 4;  // the group's first tap
    const int Ho = H * f, Wo = W * f, Q = B * H * W;
    const int q_beg = blockIdx.x * px_per_slab, q_end = min(Q, q_beg + px_per_slab);
    // (Q f f C < 2^30 elements: every byte offset below fits 32 bits)
    const __amdgpu_buffer_rsrc_t r_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, (int)((unsigned)Q * C * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_go = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(go), 0, (int)((unsigned)Q * f * f * C * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_gx = __builtin_amdgcn_make_buffer_rsrc(gx ? gx : const_cast<float*>(x), 0, gx ? (int)((unsigned)Q * C * 4u) : 0, 0x00020000);
    float4 acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int q0 = q_beg; q0 < q_end; q0 += PL) {  // (uniform per workgroup: the barriers below are reached by every thread)
        const int q = q0 + pl;
        const bool live = lane_on && q < q_end;
        const int qc = live ? q : 0;
        const int ix = qc % W, rest = qc / W, iy = rest % H, b = rest / H;
        const u32x4 rx = __builtin_amdgcn_raw_buffer_load_b128(r_x, (int)(live ? ((unsigned)qc * C4 + cq) * 16u : 0xffffffffu), 0, 0);
        float4 g[16];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int y = iy * f - p + ty0 + r, xx = ix * f - p + tx0 + c;
                const bool ok = live && (unsigned)y < (unsigned)Ho && (unsigned)xx < (unsigned)Wo;
                const u32x4 raw = __builtin_amdgcn_raw_buffer_load_b128(
                    r_go, (int)(ok ? (((unsigned)(b * Ho + y) * Wo + xx) * C4 + cq) * 16u : 0xffffffffu), 0, 0);
                g[r * 4 + c] = make_float4(__uint_as_float(raw.x), __uint_as_float(raw.y), __uint_as_float(raw.z), __uint_as_float(raw.w));
            }
        const float4 xv = make_float4(__uint_as_float(rx.x), __uint_as_float(rx.y), __uint_as_float(rx.z), __uint_as_float(rx.w));
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            acc[t].x += xv.x * g[t].x;
            acc[t].y += xv.y * g[t].y;
            acc[t].z += xv.z * g[t].z;
            acc[t].w += xv.w * g[t].w;
        }
        if (gx) {  // (uniform)
#pragma unroll
            for (int t = 0; t < 16; ++t) {  // (float4 index: the alignment is provable; a lane without a pixel holds zeros)
                const float4 wv = reinterpret_cast<const float4*>(wt)[((ty0 + (t >> 2)) * k + tx0 + (t & 3)) * C4 + cq];
                s.x += g[t].x * wv.x;
                s.y += g[t].y * wv.y;
                s.z += g[t].z * wv.z;
                s.w += g[t].w * wv.w;
            }
            if (G > 1) {
                xch[threadIdx.x] = s;
                __syncthreads();
                if (tg == 0) {
#pragma unroll
                    for (int j = 1; j < G; ++j) {
                        const float4 o = xch[j * IT + local];
                        s.x += o.x;
                        s.y += o.y;
                        s.z += o.z;
                        s.w += o.w;
                    }
                }
                __syncthreads();
            }
            const u32x4 pk = {__float_as_uint(s.x), __float_as_uint(s.y), __float_as_uint(s.z), __float_as_uint(s.w)};
            __builtin_amdgcn_raw_buffer_store_b128(pk, r_gx, (int)(live && tg == 0 ? ((unsigned)qc * C4 + cq) * 16u : 0xffffffffu), 0, 0);
        }
    }
    // the pixel lanes' accumulators, tap by tap, in lane order (lanes that own no pixel hold zeros and are not read)
    float* out = part + (size_t)blockIdx.x * kk * C;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        __syncthreads();
        xch[threadIdx.x] = acc[t];
        __syncthreads();
        if (lane_on && pl == 0) {
            float4 v = xch[tg * IT + cq];
            for (int j = 1; j < PL; ++j) {
                const float4 o = xch[tg * IT + j * C4 + cq];
                v.x += o.x;
                v.y += o.y;
                v.z += o.z;
                v.w += o.w;
            }
            const int tap = (ty0 + (t >> 2)) * k + tx0 + (t & 3);
            *reinterpret_cast<float4*>(out + (size_t)tap * C + 4 * cq) = v;
        }
    }
}

// gw[c][tap] = the slabs' part[s][tap][c] (two_level_sum)
__global__ __launch_bounds__(256) void dw_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw, int nslab, int C,
                                                              int kk) {
    __shared__ float red[256];
    const int n = kk * C, e = blockIdx.x * 32 + (threadIdx.x & 31);
    const float t = two_level_sum(red, e < n, nslab, 0.f, [&](float v, int s) { return v + part[(size_t)s * n + e]; });
    if (threadIdx.x < 32 && e < n) {
        const int tap = e / C, c = e - tap * C;
        gw[(size_t)c * kk + tap] = t;
    }
}

// Depth-wise slabs: whole pixel-lane rounds, about eight rounds per workgroup, at most 1024 slabs (monotone in B)
struct DwPlan {
    int G, PL, px_per_slab, slabs;
    size_t lds, part_bytes;
};
DwPlan dw_plan(int B, int H, int W, int C, int f) {
    DwPlan P;
    const int k = 2 * f;
    P.G = k * k / 16;
    P.PL = (256 / P.G) / (C / 4);
    const size_t Q = (size_t)B * H * W;
    const size_t rounds = (Q + P.PL - 1) / P.PL;
    const size_t want = std::max<size_t>(1, std::min<size_t>(1024, (rounds + 7) / 8));
    const size_t rps = (rounds + want - 1) / want;
    P.px_per_slab = (int)(rps * P.PL);
    P.slabs = (int)((Q + P.px_per_slab - 1) / P.px_per_slab);
    P.lds = (1024 + (size_t)k * k * C) * sizeof(float);
    P.part_bytes = want * k * k * C * sizeof(float);  // (the slab count's upper bound: monotone in B)
    return P;
}

float* dw_carve(Carve& c, const DwPlan& P) { return c.take<float>(P.part_bytes); }

struct DensePlan {
    ConvWgradPlan wg;
    int cpad;          // the data gradient's N tile padding of Cin
    bool wg16, dg16;   // f16x3: the weight gradient, the data gradient
};

// The f16x3 data gradient's launch: grad_out [B,2H,2W,Cout] (*) w read as [out = Cin][in = Cout][4][4], stride 2, pad 1, on the
// operands cp_pack_f16x3 made (`cw`); false where no f16x3 kernel takes it
bool dense_dgrad16_params(ConvParams& p, const cp_engine::ConvW& cw, const DeconvBwdArgs& a, const unsigned* go_amax) {
    p = cp_engine::conv_params(a.B, 2 * a.H, 2 * a.W, &a.go, &a.Cout, 1, cw, 2, 1, CP_ACT_NONE);
    p.dbg = 0;
    p.out = a.gx;
    p.store = CP_STORE_NHWC;
    p.ldo = a.Cin;
    return cp_engine::conv_params_f16(p, cw, &go_amax, true);
}

DensePlan dense_plan(int B, int H, int W, int Cin, int Cout, int precision) {
    DensePlan P;
    P.wg = cp_conv_wgrad_plan((size_t)B * H, Cout, Cin, 16);
    P.cpad = (int)cp_engine::align_up((size_t)Cin, cp_conv_tile_n(Cin));
    P.wg16 = precision == CP_PREC_F16X3;
    P.dg16 = false;
    if (P.wg16) {  // (host arithmetic on the launch's shape: the pointers only have to be there)
        static const float dummy = 0.f;
        cp_engine::ConvW cw = cp_engine::conv_w_f32(nullptr, nullptr, nullptr, Cout, Cin, 4, 4);
        cw.w16_hi = cw.w16_lo = (void*)&dummy;
        cw.Kpad16 = cw.K;
        const DeconvBwdArgs a{&dummy, &dummy, &dummy, nullptr, nullptr, B, H, W, Cin, Cout, 2, 1};
        ConvParams p;
        P.dg16 = dense_dgrad16_params(p, cw, a, nullptr);
    }
    return P;
}
// float32: [slab][wp], the workspace it always was.  f16x3: [slab][wp, or the data gradient's f16x3 pack][|max| slot block
// (slot 0: grad_out, slot 1: x)][grad_out split][x split]
struct DenseWs {
    float *slab, *wp;
    Pack16 f16;
    unsigned* slot;
    uint32_t *go16, *x16;
};
DenseWs dense_carve(Carve& c, const DensePlan& P, int B, int H, int W, int Cin, int Cout, bool need_gx) {
    DenseWs r{};
    r.slab = c.take<float>(P.wg.slab_bytes);
    if (need_gx && P.dg16)
        r.f16 = carve_pack16(c, (size_t)16 * Cout, (size_t)P.cpad);
    else
        r.wp = c.take<float>(need_gx ? (size_t)16 * Cout * P.cpad * 4 : 0);
    if (P.wg16) {
        r.slot = c.take<unsigned>(cp_amax_slot_bytes);
        r.go16 = c.take<uint32_t>((size_t)B * H * W * 4 * Cout * 4);
        r.x16 = c.take<uint32_t>((size_t)B * H * W * Cin * 4);
    }
    return r;
}

}  // namespace

bool cp_deconv_dw_geometry(int Cin, int Cout, int K, int stride, int pad, int groups) {
    return groups == Cin && Cin == Cout && (stride == 2 || stride == 4) && K == 2 * stride && pad == stride / 2 && Cin >= 4 &&
           Cin % 4 == 0 && (size_t)K * K * Cin * sizeof(float) <= CP_DECONV_DW_TABLE_BYTES;
}

bool cp_deconv_dense_geometry(int Cin, int Cout, int K, int stride, int pad, int groups) {
    return groups == 1 && K == 4 && stride == 2 && pad == 1 && Cin >= 32 && Cin % 32 == 0 && Cout >= 32 && Cout % 32 == 0;
}

size_t cp_deconv_backward_ws_bytes(int B, int H, int W, int Cin, int Cout, int stride, int groups, int need_grad_x, int precision) {
    Carve c{nullptr};
    if (groups != 1)
        dw_carve(c, dw_plan(B, H, W, Cin, stride));
    else
        dense_carve(c, dense_plan(B, H, W, Cin, Cout, precision), B, H, W, Cin, Cout, need_grad_x != 0);
    return c.off;
}

int cp_deconv_backward_prec_mask(int B, int H, int W, int Cin, int Cout, int groups, int precision) {
    if (groups != 1) return 0;  // (no matrix product)
    const DensePlan P = dense_plan(B, H, W, Cin, Cout, precision);
    return (P.wg16 ? 1 : 0) | (P.dg16 ? 2 : 0);
}

int cp_launch_deconv_backward(hipStream_t s, const DeconvBwdArgs& a, void* ws, int precision) {
    Carve cv{(char*)ws};
    if (a.groups != 1) {
        const DwPlan P = dw_plan(a.B, a.H, a.W, a.Cin, a.stride);
        float* part = dw_carve(cv, P);
        if (P.G == 1)
            hipLaunchKernelGGL(dw_bwd_kernel<1>, dim3(P.slabs), dim3(256), P.lds, s, a.x, a.w, a.go, a.gx, part, a.B, a.H, a.W, a.Cin,
                               a.stride, P.px_per_slab);
        else
            hipLaunchKernelGGL(dw_bwd_kernel<4>, dim3(P.slabs), dim3(256), P.lds, s, a.x, a.w, a.go, a.gx, part, a.B, a.H, a.W, a.Cin,
                               a.stride, P.px_per_slab);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        const int kk = 4 * a.stride * a.stride;
        hipLaunchKernelGGL(dw_wgrad_reduce_kernel, dim3((kk * a.Cin + 31) / 32), dim3(256), 0, s, (const float*)part, a.gw, P.slabs,
                           a.Cin, kk);
        return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
    }
    const DensePlan P = dense_plan(a.B, a.H, a.W, a.Cin, a.Cout, precision);
    const DenseWs r = dense_carve(cv, P, a.B, a.H, a.W, a.Cin, a.Cout, a.gx != nullptr);
    // f16x3: the |max| of grad_out and x, then their split copies (conv_bwd16.hip's operand form)
    const unsigned *go_amax = r.slot, *x_amax = r.slot + 1;
    if (P.wg16) {
        const size_t nx = (size_t)a.B * a.H * a.W * a.Cin, ng = (size_t)a.B * a.H * a.W * 4 * a.Cout;
        if (hipMemsetAsync(r.slot, 0, cp_amax_slot_bytes, s) != hipSuccess) return CP_ERR_LAUNCH;
        int rc = cp_launch_absmax32(a.go, ng, r.slot, s);
        if (rc == CP_OK) rc = cp_launch_absmax32(a.x, nx, r.slot + 1, s);
        if (rc == CP_OK) rc = cp_launch_split16(a.go, r.go16, ng, go_amax, s);
        if (rc == CP_OK) rc = cp_launch_split16(a.x, r.x16, nx, x_amax, s);
        if (rc != CP_OK) return rc;
    }
    // grad_w: the stride-2 convolution's weight gradient with grad_out as its input and x as its output gradient
    const ConvBwdArgs c{a.go, nullptr, nullptr, nullptr, nullptr, a.gw, nullptr, a.B, 2 * a.H, 2 * a.W, a.Cout, a.Cin, 4, 4, 2, 1};
    const ConvWgrad16 h{r.x16, r.go16, x_amax, go_amax};
    int rc = cp_launch_conv_wgrad(s, c, a.x, a.Cin, P.wg, r.slab, 0, P.wg16 ? &h : nullptr);
    if (rc != CP_OK || !a.gx) return rc;
    if (P.dg16) {
        // grad_x on the f16x3 implicit GEMM: w is already a [out = Cin][in = Cout][4][4] weight, so it is packed as a forward
        // convolution's (a power-of-two scale per row, its inverse in the epilogue); grad_out's |max| is slot 0 above
        cp_engine::ConvW cw = cp_engine::conv_w_f32(nullptr, nullptr, nullptr, a.Cout, a.Cin, 4, 4);
        rc = cp_pack_f16x3(r.f16, a.w, nullptr, 16, cw, nullptr, 0, nullptr, 0, s);
        if (rc != CP_OK) return rc;
        ConvParams d;
        if (!dense_dgrad16_params(d, cw, a, go_amax)) return CP_ERR_LAUNCH;  // (the plan asked the same question)
        return cp_launch_conv16(d, s);
    }
    // grad_x = conv2d(grad_out, w as [out = Cin][in = Cout][4][4], stride 2, pad 1), exact float32
    if (hipMemsetAsync(r.wp, 0, (size_t)16 * a.Cout * P.cpad * 4, s) != hipSuccess) return CP_ERR_LAUNCH;
    rc = cp_launch_pack_weight(a.w, r.wp, a.Cin, a.Cout, 16, a.Cout, P.cpad, 0, s);
    if (rc != CP_OK) return rc;
    const ConvParams d = grad_conv_params(a.B, 2 * a.H, 2 * a.W, a.go, a.Cout, r.wp, nullptr, a.Cin, 4, 4, 2, 1, a.gx);
    return cp_launch_conv(d, s);
}
