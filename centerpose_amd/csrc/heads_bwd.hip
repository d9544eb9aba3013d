// Backward of the prediction-head block (cp_pose_heads_backward): n heads Conv2d(Cin, hid, 3, padding=1) -> ReLU ->
// Conv2d(hid, classes_i, 1) that all read one NHWC feature map (pose_dla_dcn.py:491-521, resnet_dcn.py), with autograd's
// semantics.  Nothing is kept from the forward: a head's hidden layer is recomputed for a chunk of images, used and dropped.
//
// Per head with a gradient, per chunk of `nb` images (the hidden chunk is at most 256 MiB, or one image), on the caller's
// stream, float32 arithmetic only:
//   1. hidden   hb[q][h] = feat (*) w0 + b0, pre-activation, NHWC: the exact-f32 implicit GEMM of igemm.hip
//               (v_mfma_f32_32x32x2_f32, K = 9 Cin);
//   2. thin     one pass over hb (thin_kernel, float32 VALU): gate = hb > 0; grad_w1 += relu(hb)^T x grad_out; hb is
//               REPLACED by grad_hidden = gate * (grad_out x w1); grad_b0 += column sums of grad_hidden.  Partial sums per
//               pixel slab, slabs summed in slab order (thin_reduce_kernel);
//   3. wgrad    grad_w0 (+)= feat^T x grad_hidden: conv_bwd.hip's weight gradient (cp_launch_conv_wgrad: wgrad_kernel, K = pixels,
//               per-slab partial sums, wgrad_reduce_kernel) with gs = hb, 3x3 / stride 1 / pad 1; the first chunk writes, later
//               chunks add their finished sum to it;
//   4. dgrad    grad_feat (+)= grad_hidden (*) flipped w0^T: conv_bwd.hip's stride-1 data gradient (cp_launch_conv_dgrad_pack
//               once per head, cp_launch_conv_dgrad_s1 per chunk: the implicit GEMM of step 1 with K = 9 hid); the first head
//               writes the chunk, later heads add to it through the kernel's residual input (same stream: no atomics, no halo
//               exchange).  Skipped entirely when the caller passes no grad_feat.
//   grad_b1 = per-channel sums of grad_out in a fixed tree (cp_launch_rowsum_nchw), once per head.
// Every sum has a fixed order, so all outputs are bitwise reproducible run to run.  The hidden chunk makes one round trip
// through memory per step (write in 1, read + write in 2, read in 3 and 4): 16 MiB per image and head at 128 x 128 x 256
// against 14.5 GFLOP of contractions, i.e. a few percent of the matrix time; it is the price of building steps 1 and 4
// from the library's tuned convolution instead of a hand-fused tile pipeline.
//
// CP_PREC_F16X3 (opt-in; cp_pose_heads_backward_prec) runs the three contractions on the split-binary16 kernels; everything
// else above -- the gate, grad_w1, grad_b0, grad_b1, every slab order -- is the same float32 code:
//   0. once per call: |max| of feat (cp_launch_absmax32) and its split copy x16 (cp_launch_split16), shared by all heads and chunks;
//   1. hidden   cp_launch_conv16 on the operands cp_pose_heads_forward packs (cp_pack_f16x3) with in_amax = feat's slot: the
//               kernel, the operands and hence the values an f16x3 forward's ReLU saw;
//   2. thin     thin_kernel<CMAX, true> also commits max |grad_hidden| of the chunk into a slot (no pass of its own);
//   2b. split   gs16 = split(grad_hidden * 2^e_g) (cp_launch_split16): the one extra pass over the chunk;
//   3. wgrad    cp_launch_conv_wgrad with ConvWgrad16{gs16, x16 of the chunk, the two slots};
//   4. dgrad    cp_launch_conv_dgrad_pack(CP_PREC_F16X3) per head, cp_launch_conv_dgrad_s1(..., gs's slot) per chunk.
// Steps 1 and 4 fall back to float32, each on its own, where cp_conv16_supported refuses the launch (a chunk beyond
// 0xf0000000 bytes); cp_pose_heads_backward_mask reports what runs.  The only atomics are the order-free |max| commits.
#include "op_common.h"

#include <algorithm>

namespace {

constexpr size_t kChunkBytes = (size_t)256 << 20;  // the recomputed hidden chunk (dcn_bwd.hip's grad_col precedent)
constexpr int TL = 1024;                           // floats of one wave's grad_out tile in LDS (thin_kernel)

// One pass over the hidden chunk hb [Q][hid] (pre-activation in, grad_hidden out).  A workgroup owns `slab_px` pixels and 64
// hidden channels (lane = channel); its four waves take tiles of PT pixels in turn.  go_t [Q][cls] is the chunk's grad_out
// pixel-major; a wave stages its tile in LDS (zero-padded to CMAX channels) and reads it back as broadcasts.
// part[slab][c][h], c < cls: grad_w1 partial; c == cls: grad_b0 partial.  Sums: pixels ascending per wave, then waves 0..3.
// AMAX (f16x3): max |grad_hidden| of the slab is folded into g_slot (cp_amax_commit) -- a max beside the sums, none of them changed.
template <int CMAX, bool AMAX>
__global__ __launch_bounds__(256) void thin_kernel(float* __restrict__ hb, const float* __restrict__ go_t,
                                                   const float* __restrict__ w1, float* __restrict__ part, int Q, int hid,
                                                   int cls, int slab_px, unsigned* __restrict__ g_slot) {
    constexpr int PT = TL / CMAX < 64 ? TL / CMAX : 64;
    __shared__ float gs[4][PT * CMAX];
    __shared__ float red[(CMAX + 1) * 64];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = blockIdx.y * 64 + lane;
    const bool hv = h < hid;
    const int hc = hv ? h : 0;
    const int q_beg = blockIdx.x * slab_px, q_end = min(Q, q_beg + slab_px);
    float w1r[CMAX], acc[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        w1r[c] = (hv && c < cls) ? w1[(size_t)c * hid + hc] : 0.f;
        acc[c] = 0.f;
    }
    float gb0 = 0.f, gm = 0.f;
    for (int qb0 = q_beg; qb0 < q_end; qb0 += 4 * PT) {  // the same trip count for the four waves (barriers inside)
        const int qb = qb0 + wv * PT;
        for (int e = lane; e < PT * CMAX; e += 64) {
            const int j = e / CMAX, c = e - j * CMAX;
            const bool ok = qb + j < q_end && c < cls;
            const float v = go_t[ok ? (size_t)(qb + j) * cls + c : 0];
            gs[wv][e] = ok ? v : 0.f;
        }
        __syncthreads();
        const int np = max(0, min(PT, q_end - qb));
        for (int j0 = 0; j0 < np; j0 += 4) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = min(qb + j0 + u, q_end - 1);
                v[u] = hb[(size_t)q * hid + hc];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (j0 + u >= np) break;  // wave-uniform
                const float a = cp_relu(v[u]);
                float g = 0.f;
                const float* gr = &gs[wv][(j0 + u) * CMAX];
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    const float gc = gr[c];
                    acc[c] = fmaf(a, gc, acc[c]);
                    g = fmaf(gc, w1r[c], g);
                }
                g = cp_relu_gate(g, v[u]);
                if (hv) hb[(size_t)(qb + j0 + u) * hid + h] = g;
                gb0 += g;
                if (AMAX) gm = fmaxf(gm, fabsf(g));
            }
        }
        __syncthreads();
    }
    for (int w = 0; w < 4; ++w) {
        if (wv == w) {
#pragma unroll
            for (int c = 0; c < CMAX; ++c) red[c * 64 + lane] = w ? red[c * 64 + lane] + acc[c] : acc[c];
            red[CMAX * 64 + lane] = w ? red[CMAX * 64 + lane] + gb0 : gb0;
        }
        __syncthreads();
    }
    if (AMAX) cp_amax_commit(g_slot, gm);  // (pad lanes h >= hid: w1r = 0, so g = 0)
    if (!hv) return;
    float* out = part + (size_t)blockIdx.x * (cls + 1) * hid;
    for (int c = wv; c <= cls; c += 4) out[(size_t)c * hid + h] = red[(c < cls ? c : CMAX) * 64 + lane];
}

// gw1[c][h] and gb0[h] = the slabs' partials by serial_sum.  `accum`: the sum STARTS from the value already there (a later chunk
// of the batch continues the earlier chunks' chain), otherwise from zero.
__global__ void thin_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw1, float* __restrict__ gb0, int nslab,
                                   int cls, int hid, int accum) {
    const int n = (cls + 1) * hid;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        float* dst = e < cls * hid ? gw1 + e : gb0 + (e - cls * hid);
        *dst = serial_sum(part, nslab, (size_t)n, (size_t)e, accum ? *dst : 0.f);
    }
}

struct Plan {
    int nb;                   // images per chunk
    int hpad;                 // hid padded to the hidden convolution's N tile
    int thin_px, thin_slabs;  // thin_kernel: pixels per slab, slabs of a full chunk
    ConvWgradPlan wg;         // the weight gradient of a full chunk
    bool wg16, dg16, hid16;   // f16x3: the weight gradient, the data gradient, the recomputed hidden layer
};

// The hidden layer's launch: pre-activation, NHWC.  `cw` carries the f16x3 operands when the launch is to go to cp_launch_conv16;
// dbg = 0 as every convolution of a gradient (grad_conv_params).
ConvParams hidden_params(int nb, int H, int W, const float* fc, int Cin, const cp_engine::ConvW& cw, float* hb) {
    ConvParams p = cp_engine::conv_params(nb, H, W, &fc, &Cin, 1, cw, 1, 1, CP_ACT_NONE);
    p.dbg = 0;
    p.out = hb;
    p.store = CP_STORE_NHWC;
    p.ldo = cw.Cout;
    return p;
}

// would cp_launch_conv16 take the hidden layer of a full chunk?  (host arithmetic on the launch's shape: the pointers only have
// to be there)
bool hidden16_supported(int nb, int H, int W, int Cin, int hid) {
    static float dummy = 0.f;
    cp_engine::ConvW cw = cp_engine::conv_w_f32(&dummy, nullptr, &dummy, Cin, hid, 3, 3);
    cw.w16_hi = cw.w16_lo = &dummy;
    cw.Kpad16 = cw.K;
    ConvParams p = hidden_params(nb, H, W, &dummy, Cin, cw, &dummy);
    const unsigned* none = nullptr;
    return cp_engine::conv_params_f16(p, cw, &none, true);
}

Plan plan(int B, int H, int W, int Cin, int hid, int precision) {
    Plan P;
    const size_t HW = (size_t)H * W;
    P.nb = cp_pose_heads_chunk(B, H, W, hid);
    P.hpad = (int)((hid + cp_conv_tile_n(hid) - 1) / cp_conv_tile_n(hid) * cp_conv_tile_n(hid));
    const size_t Q = (size_t)P.nb * HW;
    // thin: about two workgroups per CU and channel group, at least 256 pixels a slab
    size_t ts = std::max<size_t>(1, std::min<size_t>(512, (Q + 255) / 256));
    P.thin_px = (int)((Q + ts - 1) / ts);
    P.thin_slabs = (int)((Q + P.thin_px - 1) / P.thin_px);
    P.wg = cp_conv_wgrad_plan((size_t)P.nb * H, Cin, hid, 9);
    // f16x3: the weight gradient always (3x3 / stride 1 / pad 1, Cin % 32 == 0); the two igemm16.hip launches where that file
    // takes a full chunk (32-bit byte offsets)
    P.wg16 = precision == CP_PREC_F16X3;
    P.dg16 = P.wg16 && cp_conv_dgrad16_s1_supported(P.nb, H, W, Cin, hid, 3);
    P.hid16 = P.wg16 && hidden16_supported(P.nb, H, W, Cin, hid);
    return P;
}

// wA [9 Cin][hpad] and shift [hpad] are adjacent: one memset clears both
struct Ws {
    float *wA, *shift, *wB, *hb, *go_t, *part, *slab;
    // f16x3: the hidden layer's packed operands, the |max| slot blocks of feat and of the chunk's grad_hidden, the split copies
    // of the chunk's grad_hidden and of the WHOLE feature map (made once per call), the data gradient's packed weight
    Pack16 w16;
    unsigned *x_slot, *g_slot;
    uint32_t *gs16, *x16;
    float* wB16;
};
Ws heads_bwd_carve(Carve& c, const Plan& P, int B, int H, int W, int Cin, int hid, int cmax) {
    const size_t Q = (size_t)P.nb * H * W;
    Ws r;
    r.wA = c.take<float>((size_t)9 * Cin * P.hpad * 4);
    r.shift = c.take<float>((size_t)P.hpad * 4);
    r.wB = c.take<float>(cp_conv_dgrad_pack_bytes(Cin, hid, 9, CP_PREC_F32));
    r.hb = c.take<float>(Q * hid * 4);
    r.go_t = c.take<float>(Q * cmax * 4);
    r.part = c.take<float>((size_t)P.thin_slabs * (cmax + 1) * hid * 4);
    r.slab = c.take<float>(P.wg.slab_bytes);
    r.w16 = Pack16{};
    r.x_slot = r.g_slot = nullptr;
    r.gs16 = r.x16 = nullptr;
    r.wB16 = nullptr;
    if (P.wg16) {  // (nothing is taken in float32: that workspace is the one it always was)
        r.w16 = carve_pack16(c, (size_t)9 * Cin, (size_t)P.hpad);  // (also where the hidden layer stays float32: monotone in B)
        r.x_slot = c.take<unsigned>(cp_amax_slot_bytes);
        r.g_slot = c.take<unsigned>(cp_amax_slot_bytes);
        r.gs16 = c.take<uint32_t>(Q * hid * 4);
        r.x16 = c.take<uint32_t>((size_t)B * H * W * Cin * 4);
        r.wB16 = c.take<float>(P.dg16 ? cp_conv_dgrad_pack_bytes(Cin, hid, 9, CP_PREC_F16X3) : 0);
    }
    return r;
}

}  // namespace

int cp_pose_heads_chunk(int B, int H, int W, int hid) {
    const size_t per_img = (size_t)H * W * hid * 4;
    const size_t cap = std::min<size_t>(kChunkBytes / per_img, 16384);  // (the layout kernels put the chunk's images on grid z)
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)B, cap));
}

size_t cp_pose_heads_backward_ws_bytes(int B, int H, int W, int Cin, int hid, int max_classes, int precision) {
    Carve c{nullptr};
    heads_bwd_carve(c, plan(B, H, W, Cin, hid, precision), B, H, W, Cin, hid, max_classes);
    return c.off;
}

int cp_pose_heads_backward_mask(int B, int H, int W, int Cin, int hid, int precision) {
    const Plan P = plan(B, H, W, Cin, hid, precision);
    return (P.wg16 ? 1 : 0) | (P.dg16 ? 2 : 0) | (P.hid16 ? 4 : 0);
}

int cp_launch_pose_heads_backward(hipStream_t s, const PoseHeadsArgs& a, const float* const* grad_out, float* const* grad_w0,
                                  float* const* grad_b0, float* const* grad_w1, float* const* grad_b1, float* grad_feat,
                                  void* ws, int precision) {
    int cmax = 1;
    for (int i = 0; i < a.n; ++i) cmax = std::max(cmax, a.classes[i]);
    const Plan P = plan(a.B, a.H, a.W, a.Cin, a.hid, precision);
    Carve cv{(char*)ws};
    const Ws r = heads_bwd_carve(cv, P, a.B, a.H, a.W, a.Cin, a.hid, cmax);
    float *wA = r.wA, *shift = r.shift, *wB = r.wB, *hb = r.hb, *go_t = r.go_t, *part = r.part, *slab = r.slab;
    const int B = a.B, H = a.H, W = a.W, Cin = a.Cin, hid = a.hid, HW = H * W;
    bool feat_written = false, feat_split = false;
    for (int i = 0; i < a.n; ++i) {
        const int cls = a.classes[i];
        if (!grad_out[i]) {  // a head the loss does not use: zero parameter gradients, nothing added to grad_feat
            if (hipMemsetAsync(grad_w0[i], 0, (size_t)hid * Cin * 9 * 4, s) != hipSuccess ||
                hipMemsetAsync(grad_b0[i], 0, (size_t)hid * 4, s) != hipSuccess ||
                hipMemsetAsync(grad_w1[i], 0, (size_t)cls * hid * 4, s) != hipSuccess ||
                hipMemsetAsync(grad_b1[i], 0, (size_t)cls * 4, s) != hipSuccess)
                return CP_ERR_LAUNCH;
            continue;
        }
        // the head's packed operands: wA [9 Cin][hpad] and b0 padded for the hidden layer, wB for the data gradient
        if (hipMemsetAsync(wA, 0, (char*)wB - (char*)wA, s) != hipSuccess) return CP_ERR_LAUNCH;
        cp_engine::ConvW cw = cp_engine::conv_w_f32(wA, nullptr, shift, Cin, hid, 3, 3);
        int rc = P.hid16 ? cp_pack_f16x3(r.w16, a.w0[i], nullptr, 9, cw, nullptr, 0, nullptr, 0, s)
                         : cp_launch_pack_weight(a.w0[i], wA, hid, Cin, 9, Cin, P.hpad, 0, s);
        if (rc != CP_OK) return rc;
        if (hipMemcpyAsync(shift, a.b0[i], (size_t)hid * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return CP_ERR_LAUNCH;
        if (grad_feat) {
            rc = P.dg16 ? cp_launch_conv_dgrad_pack(s, a.w0[i], r.wB16, Cin, hid, hid, 9, CP_PREC_F16X3)
                        : cp_launch_conv_dgrad_pack(s, a.w0[i], wB, Cin, hid, hid, 9, CP_PREC_F32);
            if (rc != CP_OK) return rc;
        }
        if (P.wg16 && !feat_split) {  // f16x3 step 0, before the first head that needs it
            const size_t nx = (size_t)B * HW * Cin;
            if (hipMemsetAsync(r.x_slot, 0, cp_amax_slot_bytes, s) != hipSuccess) return CP_ERR_LAUNCH;
            rc = cp_launch_absmax32(a.feat, nx, r.x_slot, s);
            if (rc == CP_OK) rc = cp_launch_split16(a.feat, r.x16, nx, r.x_slot, s);
            if (rc != CP_OK) return rc;
            feat_split = true;
        }
        rc = cp_launch_rowsum_nchw(grad_out[i], grad_b1[i], B, cls, HW, s);
        if (rc != CP_OK) return rc;
        for (int b0 = 0; b0 < B; b0 += P.nb) {
            const int nb = std::min(P.nb, B - b0), Q = nb * HW, accum = b0 > 0;
            const float* fc = a.feat + (size_t)b0 * HW * Cin;
            float* gf = grad_feat ? grad_feat + (size_t)b0 * HW * Cin : nullptr;
            // 1. hidden (pre-activation)
            ConvParams p = hidden_params(nb, H, W, fc, Cin, cw, hb);
            const unsigned* x_amax = r.x_slot;
            rc = P.hid16 && cp_engine::conv_params_f16(p, cw, &x_amax, true) ? cp_launch_conv16(p, s) : cp_launch_conv(p, s);
            if (rc != CP_OK) return rc;
            // 2. thin
            rc = cp_launch_nchw_to_nhwc(grad_out[i] + (size_t)b0 * cls * HW, go_t, nb, cls, H, W, cls, s);
            if (rc != CP_OK) return rc;
            const int tslabs = (Q + P.thin_px - 1) / P.thin_px;
            const dim3 tg(tslabs, (hid + 63) / 64);
            if (P.wg16 && hipMemsetAsync(r.g_slot, 0, cp_amax_slot_bytes, s) != hipSuccess) return CP_ERR_LAUNCH;
#define CP_THIN(CMAX, AMAX)                                                                                                      \
    hipLaunchKernelGGL((thin_kernel<CMAX, AMAX>), tg, dim3(256), 0, s, hb, (const float*)go_t, a.w1[i], part, Q, hid, cls, P.thin_px, \
                       r.g_slot)
            if (cls <= 4) {
                if (P.wg16) CP_THIN(4, true);
                else CP_THIN(4, false);
            } else if (cls <= 16) {
                if (P.wg16) CP_THIN(16, true);
                else CP_THIN(16, false);
            } else {
                if (P.wg16) CP_THIN(64, true);
                else CP_THIN(64, false);
            }
#undef CP_THIN
            if (!launch_ok()) return CP_ERR_LAUNCH;
            hipLaunchKernelGGL(thin_reduce_kernel, dim3(((cls + 1) * hid + 255) / 256), dim3(256), 0, s, (const float*)part,
                               grad_w1[i], grad_b0[i], tslabs, cls, hid, accum);
            if (!launch_ok()) return CP_ERR_LAUNCH;
            // 3. grad_w0 and 4. grad_feat of the chunk: the 3x3 layer's Conv2d backward on gs = grad_hidden (hid % 32 == 0: nothing
            // to stage).  grad_feat is written by the first head with a gradient and added to by the others.
            const ConvBwdArgs c{fc, a.w0[i], nullptr, nullptr, gf, grad_w0[i], nullptr, nb, H, W, Cin, hid, 3, 3, 1, 1};
            if (P.wg16) {
                rc = cp_launch_split16(hb, r.gs16, (size_t)Q * hid, r.g_slot, s);
                if (rc != CP_OK) return rc;
            }
            const ConvWgrad16 h16{r.gs16, P.wg16 ? r.x16 + (size_t)b0 * HW * Cin : nullptr, r.g_slot, r.x_slot};
            rc = cp_launch_conv_wgrad(s, c, hb, hid, P.wg, slab, accum, P.wg16 ? &h16 : nullptr);
            if (rc == CP_OK && gf)
                rc = P.dg16 ? cp_launch_conv_dgrad_s1(s, c, hb, hid, r.wB16, feat_written ? gf : nullptr, r.g_slot)
                            : cp_launch_conv_dgrad_s1(s, c, hb, hid, wB, feat_written ? gf : nullptr);
            if (rc != CP_OK) return rc;
        }
        feat_written = true;
    }
    if (grad_feat && !feat_written && hipMemsetAsync(grad_feat, 0, (size_t)B * HW * Cin * 4, s) != hipSuccess) return CP_ERR_LAUNCH;
    return CP_OK;
}
