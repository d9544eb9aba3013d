// The stand-alone operators of the C ABI (include/centerpose_hip.h): single layers on caller tensors, outside any cp_model
// -- cp_conv2d_nhwc / cp_conv2d_backward_nhwc / cp_conv2d_backward_prec_nhwc, cp_batchnorm_forward_nhwc / _backward_nhwc, cp_conv_transpose2d_nhwc,
// cp_conv_transpose2d_dw_nhwc / cp_conv_transpose2d_backward_nhwc / cp_conv_transpose2d_backward_prec_nhwc, cp_dcnv2_forward / cp_dcnv2_backward / cp_dcnv2_backward_det / cp_dcnv2_backward_prec, cp_pose_heads_forward / _backward / _backward_prec,
// cp_maxpool2d_forward_nhwc / _backward_nhwc, cp_upsample2_add_nhwc / cp_upsample2_add_backward_nhwc (large_hourglass.py:95-112),
// cp_conv2d_stem_backward / cp_conv2d_stem_wide_backward, cp_groupnorm_forward_nhwc / _backward_nhwc,
// cp_gru_gate_forward / _backward, cp_adam_table_bytes / _table_build / _step, cp_grad_flat_elems / _flat_offsets / _pack_table_bytes / _pack_table_build / _pack.
// Each packs its PyTorch-layout weights into a caller-provided workspace on every call and then launches the same kernels as
// the engine.
#include "op_common.h"

using namespace cp_engine;

namespace {

constexpr size_t kSlotBytes = cp_amax_slot_bytes;  // one |max| slot block

__global__ void dcn_offmask_pack_kernel(const float* __restrict__ offset, const float* __restrict__ mask,
                                        float* __restrict__ om, int B, int HW) {
    // offset [B,18,HW], mask [B,9,HW] -> om [B,HW,32]
    const size_t total = (size_t)B * HW * 32;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i & 31);
        const size_t px = i >> 5;
        const size_t b = px / HW, p = px - b * HW;
        float v = 0.f;
        if (c < 18) v = offset[(b * 18 + c) * HW + p];
        else if (c < 27) v = mask[(b * 9 + (c - 18)) * HW + p];
        om[i] = v;
    }
}

// max |mask| of the packed records (channels 18 .. 26) -> `slot`
__global__ void dcn_mask_amax_kernel(const float* __restrict__ om, size_t px, unsigned* __restrict__ slot) {
    float m = 0.f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < px * 9; i += (size_t)gridDim.x * blockDim.x)
        m = fmaxf(m, fabsf(om[(i / 9) * 32 + 18 + i % 9]));
    cp_amax_commit(slot, m);
}

// The f16x3 DCN kernels fold the mask into the corner weights of the pre-scaled activation, so the blended value is bounded
// by max |x| * max |mask|, not max |x|: a caller-supplied mask above 1 would push it past binary16's range (hi half saturated,
// lo half infinite).  Raise x's bound to max |x| * max(1, max |mask|), rounded up; masks within [-1, 1] leave it untouched.
__global__ void dcn_act_bound_kernel(unsigned* __restrict__ x_slot, const unsigned* __restrict__ mask_slot) {
    if (threadIdx.x != 0) return;
    const float am = __uint_as_float(cp_amax_read(mask_slot));
    if (!(am > 1.f)) return;
    const double d = (double)__uint_as_float(cp_amax_read(x_slot)) * (double)am;  // exact (24 + 24 bits)
    float bound = (float)d;
    if ((double)bound < d) bound = __uint_as_float(__float_as_uint(bound) + 1u);  // rounded up
    x_slot[0] = max(x_slot[0], __float_as_uint(bound));
}

// One convolution's operands in an operator's workspace.  The float32 ones back to back, so that one memset zeroes all `bytes`
// of them: the packed weight [kpad][cpad] and the epilogue vectors, cpad floats each because the kernels read them up to the
// N tile (scale: only where the operator takes one).  Then the f16x3 regions, where the operator has that form.
struct ConvOps {
    float *wp, *scale, *shift;
    size_t bytes;
    Pack16 f16;
};
ConvOps carve_conv_ops(Carve& c, size_t kpad, size_t cpad, bool with_scale, bool with_f16) {
    const size_t start = c.off;
    ConvOps r{};
    r.wp = c.take<float>(kpad * cpad * sizeof(float));
    r.scale = with_scale ? c.take<float>(cpad * sizeof(float)) : nullptr;
    r.shift = c.take<float>(cpad * sizeof(float));
    r.bytes = c.off - start;
    if (with_f16) r.f16 = carve_pack16(c, kpad, cpad);
    return r;
}

// What cp_conv2d_nhwc, cp_dcnv2_forward and each layer of cp_pose_heads_forward do with a PyTorch-layout weight `w`
// ([Cout][Cin][KH][KW]) before they launch: zero the regions `r`, pack the weight, copy the Cout floats of each given
// epilogue vector into its zero-padded region and, with `f16x3` (the caller chose those kernels), pack their operands from
// the same weight and measure the input (cp_pack_f16x3: x, nx, om, px).  `cw` describes the staged operands.
int stage_conv(ConvW& cw, const ConvOps& r, bool f16x3, const float* w, const float* scale, const float* shift, int Cin,
               int Cout, int KH, int KW, const float* x, size_t nx, const float* om, size_t px, hipStream_t s) {
    cw = conv_w_f32(r.wp, scale ? r.scale : nullptr, shift ? r.shift : nullptr, Cin, Cout, KH, KW);
    if (hipMemsetAsync(r.wp, 0, r.bytes, s) != hipSuccess) return CP_ERR_LAUNCH;
    const int rc = cp_launch_pack_weight(w, r.wp, Cout, Cin, KH * KW, Cin, cw.CoutPad, 0, s);
    if (rc != CP_OK) return rc;
    if ((scale && hipMemcpyAsync(r.scale, scale, (size_t)Cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) ||
        (shift && hipMemcpyAsync(r.shift, shift, (size_t)Cout * 4, hipMemcpyDeviceToDevice, s) != hipSuccess))
        return CP_ERR_LAUNCH;
    return f16x3 ? cp_pack_f16x3(r.f16, w, scale, KH * KW, cw, x, nx, om, px, s) : CP_OK;
}

// Launches `p`, built from stage_conv's `cw`: on the f16x3 kernels with `f16x3` where they take the launch, else in float32
int launch_conv(ConvParams& p, const ConvW& cw, const ConvOps& r, bool f16x3, hipStream_t s) {
    const unsigned* slot = r.f16.slot;
    return f16x3 && conv_params_f16(p, cw, &slot, true) ? cp_launch_conv16(p, s) : cp_launch_conv(p, s);
}

// cp_conv2d_nhwc: the float32 operands (scale and shift included) + the f16x3 regions
ConvOps conv2d_carve(Carve& c, int Cin, int Cout, int KH, int KW) {
    return carve_conv_ops(c, align_up((size_t)KH * KW * Cin, 16), align_up((size_t)Cout, cp_conv_tile_n(Cout)), true, true);
}

// cp_conv_transpose2d_nhwc: float32 sub-kernels + two binary16 copies + 2^-e per row + scale * 2^-e + the input's |max| slot
struct DeconvWs {
    float* wf;
    void *hi, *lo;
    float *inv, *sc16;
    unsigned* slot;
};
DeconvWs deconv_carve(Carve& c, int Cin, int Cout) {
    const size_t cpad = (size_t)cp_deconv_cout_pad(Cout > 0 ? Cout : 1), n = 4 * cpad * 4 * (size_t)(Cin > 0 ? Cin : 0);
    DeconvWs r;
    r.wf = c.take<float>(n * 4);
    r.hi = c.take<void>(n * 2);
    r.lo = c.take<void>(n * 2);
    r.inv = c.take<float>(cpad * 4);
    r.sc16 = c.take<float>(cpad * 4);
    r.slot = c.take<unsigned>(kSlotBytes);
    return r;
}

// cp_dcnv2_forward (fast path): [x NHWC B*H*W*C][offmask NHWC B*H*W*32][y NHWC B*H*W*Co][packed weights][shift cpad] + the
// f16x3 regions
struct DcnWs {
    float *x, *om, *y;
    ConvOps ops;
};
DcnWs dcn_carve(Carve& c, int B, int C, int H, int W, int Co) {
    const size_t px = (size_t)B * H * W;
    const size_t cpad = align_up((size_t)Co, cp_conv_tile_n(Co));
    DcnWs r;
    r.x = c.take<float>(px * C * 4);
    r.om = c.take<float>(px * 32 * 4);
    r.y = c.take<float>(px * Co * 4);
    r.ops = carve_conv_ops(c, (size_t)9 * C, cpad, false, true);
    return r;
}

// DCNv2 backward: shape checks here (as the forward's), kernels in dcn_bwd.hip
const char* dcn_bwd_shape_error(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                                int dw, int dg, int* Ho, int* Wo) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || Co < 1 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 || dh < 1 ||
        dw < 1 || dg < 1 || C % dg != 0)
        return "dcn_v2_backward: bad shape argument (C must be divisible by deformable_group)";
    const long long ho = ((long long)H + 2LL * ph - ((long long)dh * (kh - 1) + 1)) / sh + 1;
    const long long wo = ((long long)W + 2LL * pw - ((long long)dw * (kw - 1) + 1)) / sw + 1;
    if (ho < 1 || wo < 1 || H + 2LL * ph < (long long)dh * (kh - 1) + 1 || W + 2LL * pw < (long long)dw * (kw - 1) + 1)
        return "dcn_v2_backward: empty output (kernel extent larger than the padded input)";
    const long long lim = 0x7fffffffLL, T = (long long)kh * kw;
    if ((long long)B * C * H * W >= lim || (long long)B * Co * ho * wo >= lim || (long long)B * dg * 2 * T * ho * wo >= lim ||
        (long long)Co * C * T >= lim || (long long)C * T * ho * wo >= lim)
        return "dcn_v2_backward: a tensor has 2^31 elements or more";
    *Ho = (int)ho;
    *Wo = (int)wo;
    return nullptr;
}

// Prediction-head block (cp_pose_heads_forward / _backward): shape checks shared by the calls and their workspace queries
const char* heads_shape_error(int B, int H, int W, int Cin, int hid, int n, const int* classes, int* cmax) {
    if (n < 1 || !classes) return "pose_heads: at least one head (and its class count) is needed";
    if (B < 1 || H < 1 || W < 1) return "pose_heads: B, H and W must be at least 1";
    if (Cin < 32 || Cin % 32) return "pose_heads: Cin must be a positive multiple of 32";
    if (hid < 32 || hid % 32) return "pose_heads: the hidden width must be a positive multiple of 32";
    int mx = 0;
    for (int i = 0; i < n; ++i) {
        if (classes[i] < 1 || classes[i] > 64) return "pose_heads: classes must be in 1..64 for every head";
        mx = std::max(mx, classes[i]);
    }
    const long long lim = 0x7fffffffLL, px = (long long)B * H * W;
    if (px * Cin >= lim || px * mx >= lim || (long long)H * W * hid >= lim || (long long)hid * Cin * 9 >= lim)
        return "pose_heads: a tensor has 2^31 elements or more";
    *cmax = mx;
    return nullptr;
}

// Conv2d backward: shape checks shared by the call and its workspace query, kernels in conv_bwd.hip
const char* conv_bwd_shape_error(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    if (B < 1 || H < 1 || W < 1 || Cout < 1) return "conv2d_backward: B, H, W and Cout must be at least 1";
    if (Cin < 4 || Cin % 4) return "conv2d_backward: Cin must be a positive multiple of 4";
    if (KH < 1 || KH > 7 || KW < 1 || KW > 7 || stride < 1 || stride > 4 || pad < 0 || pad >= KH || pad >= KW)
        return "conv2d_backward: unsupported geometry (KH, KW in 1..7, stride in 1..4, 0 <= pad < K)";
    if (H + 2 * pad < KH || W + 2 * pad < KW) return "conv2d_backward: empty output (kernel extent larger than the padded input)";
    const long long ho = (H + 2 * pad - KH) / stride + 1, wo = (W + 2 * pad - KW) / stride + 1;
    const long long lim = 0x7fffffffLL, cop = ((long long)Cout + 31) / 32 * 32;
    if ((long long)B * H * W * Cin >= lim || (long long)B * ho * wo * cop >= lim || cop * Cin * KH * KW >= lim)
        return "conv2d_backward: a tensor has 2^31 elements or more";
    return nullptr;
}

// ConvTranspose2d backward and the depth-wise forward: shape checks shared by the calls and the workspace query, kernels in
// deconv_bwd.hip and ewise.hip
const char* deconv_shape_error(int B, int H, int W, int Cin, int Cout, int K, int stride, int pad, int groups) {
    if (B < 1 || H < 1 || W < 1) return "conv_transpose2d: B, H and W must be at least 1";
    const bool dw = cp_deconv_dw_geometry(Cin, Cout, K, stride, pad, groups);
    if (!dw && !cp_deconv_dense_geometry(Cin, Cout, K, stride, pad, groups))
        return "conv_transpose2d: unsupported geometry (depth-wise: groups == Cin == Cout, stride 2 or 4, K == 2 stride, pad == "
               "stride / 2, C % 4 == 0, K K C floats within the LDS table; dense: groups 1, K 4, stride 2, pad 1, Cin and Cout "
               "multiples of 32)";
    // (the depth-wise kernels address their tensors through 32-bit byte offsets: 2^30 elements)
    const long long lim = dw ? 0x40000000LL : 0x7fffffffLL, px = (long long)B * H * W;
    if (px * Cin >= lim || px * stride * stride * Cout >= lim || (long long)Cin * (Cout / groups) * K * K >= lim)
        return dw ? "conv_transpose2d: a tensor has 2^30 elements or more (the depth-wise kernels' limit)"
                  : "conv_transpose2d: a tensor has 2^31 elements or more";
    return nullptr;
}

// BatchNorm: shape checks shared by the two calls and their workspace query, kernels in batchnorm.hip
const char* bn_shape_error(int B, int H, int W, int C) {
    if (B < 1 || H < 1 || W < 1) return "batchnorm: B, H and W must be at least 1";
    if (C < 4 || C > 4096 || C % 4) return "batchnorm: C must be a multiple of 4 in 4..4096";
    if ((long long)B * H * W * C >= 0x7fffffffLL) return "batchnorm: a tensor has 2^31 elements or more";
    return nullptr;
}
// the kernels read and write 16 bytes per lane
bool bn_aligned(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((uintptr_t)p & 15) return false;
    return true;
}

// GroupNorm: shape checks shared by the two calls and their workspace query, kernels in groupnorm.hip
const char* gn_shape_error(int B, int H, int W, int C, int G) {
    if (B < 1 || H < 1 || W < 1) return "groupnorm: B, H and W must be at least 1";
    if (C < 4 || C > 4096 || C % 4) return "groupnorm: C must be a multiple of 4 in 4..4096";
    if (G < 1 || C % G) return "groupnorm: G must be at least 1 and divide C";
    if (C / G != 1 && C / G != 2 && (C / G) % 4)
        return "groupnorm: C / G must be 1, 2 or a multiple of 4 (a lane's four channels must not straddle a group unevenly)";
    if ((long long)B * H * W * C >= 0x7fffffffLL) return "groupnorm: a tensor has 2^31 elements or more";
    return nullptr;
}
// the GRU gate: x3 [M][3 Ch] is the largest tensor
const char* gru_shape_error(int M, int Ch) {
    if (M < 1) return "gru_gate: M must be at least 1";
    if (Ch < 4 || Ch > 1024 || Ch % 4) return "gru_gate: Ch must be a multiple of 4 in 4..1024";
    if ((long long)M * 3 * Ch >= 0x7fffffffLL) return "gru_gate: a tensor has 2^31 elements or more";
    return nullptr;
}

// The precision argument of the backward passes that take one (`op`: conv2d_backward, conv_transpose2d_backward, pose_heads_backward, dcn_v2_backward)
std::string prec_error(const char* op, int precision) {
    if (precision == CP_PREC_F32 || precision == CP_PREC_F16X3) return std::string();
    return std::string(op) + ": unknown precision (CP_PREC_F32 or CP_PREC_F16X3)";
}
// What every entry of such an operator checks first, in this order: its shape (the operator's *_shape_error), then the
// precision.  Records the first refusal in cp_last_error and returns true.
bool refused(const char* shape_error, const char* op, int precision) {
    const std::string e = shape_error ? std::string(shape_error) : prec_error(op, precision);
    if (!e.empty()) fail(CP_ERR_INVALID, e);
    return !e.empty();
}

// cp_pose_heads_forward: per head the 3x3 layer's float32 and f16x3 operands + bias, the 1x1 layer's, one hidden chunk
struct HeadsFwdWs {
    ConvOps ops0, ops1;
    float* hid;
};
HeadsFwdWs heads_fwd_carve(Carve& c, int B, int H, int W, int Cin, int hid) {
    const size_t k0 = (size_t)9 * Cin, hpad = align_up((size_t)hid, cp_conv_tile_n(hid));
    HeadsFwdWs r;
    r.ops0 = carve_conv_ops(c, k0, hpad, false, true);
    r.ops1 = carve_conv_ops(c, (size_t)hid, 64, false, false);
    r.hid = c.take<float>((size_t)cp_pose_heads_chunk(B, H, W, hid) * H * W * hid * 4);
    return r;
}

}  // namespace

// Packs the PyTorch-layout weight `wt` ([w.Cout][w.Cin][taps]) for the f16x3 path into the carved regions `r` and measures the
// input: range-safe operands -- per-channel power-of-two weight scale (folded into scale16 with `scale`), per-tensor activation
// scale from one |max| pass over x[0..nx) (x == nullptr: the caller measures the input into a slot block of its own and r.slot
// stays zero).  `om` (DCN: the packed offset / mask records of `px` pixels): the mask's |max| goes to slot 1 of the (zeroed) slot
// block and is folded into x's bound.  The fragment-ordered copies exist when the shape allows them.  On CP_OK the f16x3
// fields of `w` describe the packed operands.  Declared in op_common.h: heads_bwd.hip packs its recomputed hidden layer with it.
int cp_pack_f16x3(const Pack16& r, const float* wt, const float* scale, int taps, ConvW& w, const float* x, size_t nx,
                  const float* om, size_t px, hipStream_t s) {
    if (hipMemsetAsync(r.hi, 0, (char*)r.wfwd - (char*)r.hi, s) != hipSuccess) return CP_ERR_LAUNCH;
    if (hipMemsetAsync(r.wfwd, 0, (char*)r.fhi - (char*)r.wfwd, s) != hipSuccess) return CP_ERR_LAUNCH;
    w.w16_hi = r.hi;
    w.w16_lo = r.lo;
    w.Kpad16 = w.K;
    w.scale16 = r.sc16;
    int rc = cp_launch_weight_scale(wt, w.Cout, w.Cin * taps, r.wfwd, r.winv, s);
    if (rc == CP_OK) rc = cp_launch_pack_weight16(wt, r.hi, r.lo, w.Cout, w.Cin, taps, w.Kpad16, 0, r.wfwd, s);
    if (rc == CP_OK) rc = cp_launch_scale16(scale, r.winv, r.sc16, w.Cout, s);
    if (rc == CP_OK && x) rc = cp_launch_absmax(x, nx, r.slot, s);
    if (rc == CP_OK && om) {
        const size_t g = std::min<size_t>((px * 9 + 255) / 256, 2048);
        hipLaunchKernelGGL(dcn_mask_amax_kernel, dim3((unsigned)g), dim3(256), 0, s, om, px, r.slot + 1);
        hipLaunchKernelGGL(dcn_act_bound_kernel, dim3(1), dim3(64), 0, s, r.slot, (const unsigned*)(r.slot + 1));
        if (hipGetLastError() != hipSuccess) rc = CP_ERR_LAUNCH;
    }
    if (rc == CP_OK && w.CoutPad % 32 == 0 && w.Kpad16 % 16 == 0) {
        rc = cp_launch_frag16_repack(r.hi, r.fhi, w.CoutPad, w.Kpad16, s);
        if (rc == CP_OK) rc = cp_launch_frag16_repack(r.lo, r.flo, w.CoutPad, w.Kpad16, s);
        w.w16f_hi = r.fhi;
        w.w16f_lo = r.flo;
    }
    return rc;
}

extern "C" {

int cp_pose_heads_chunk_images(int B, int H, int W, int hid) {
    if (B < 1 || H < 1 || W < 1 || hid < 1) return 0;
    return cp_pose_heads_chunk(B, H, W, hid);
}

size_t cp_pose_heads_forward_workspace_bytes(int B, int H, int W, int Cin, int hid, int n, const int* classes) {
    int cmax = 0;
    if (const char* e = heads_shape_error(B, H, W, Cin, hid, n, classes, &cmax)) {
        fail(CP_ERR_INVALID, e);
        return 0;
    }
    Carve c{nullptr};
    heads_fwd_carve(c, B, H, W, Cin, hid);
    return c.off;
}

int cp_pose_heads_forward(cp_stream_t stream, const float* feat, int n, const float* const* w0, const float* const* b0,
                          const float* const* w1, const float* const* b1, const int* classes, float* const* out, int B, int H,
                          int W, int Cin, int hid, void* workspace, size_t workspace_bytes) {
    int cmax = 0;
    if (const char* e = heads_shape_error(B, H, W, Cin, hid, n, classes, &cmax)) return fail(CP_ERR_INVALID, e);
    if (!feat || !w0 || !b0 || !w1 || !b1 || !out || !workspace) return fail(CP_ERR_INVALID, "pose_heads_forward: null argument");
    for (int i = 0; i < n; ++i)
        if (!w0[i] || !b0[i] || !w1[i] || !b1[i] || !out[i]) return fail(CP_ERR_INVALID, "pose_heads_forward: null argument");
    Carve c{(char*)workspace};
    const HeadsFwdWs r = heads_fwd_carve(c, B, H, W, Cin, hid);
    if (workspace_bytes < c.off) return fail(CP_ERR_INVALID, "pose_heads_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W, chunk = cp_pose_heads_chunk(B, H, W, hid);
    // range-safe f16x3 operands of the 3x3 layer, as cp_conv2d_nhwc builds them; the 1x1 layer stays exact
    const bool f16x3 = g_default_precision == CP_PREC_F16X3;
    for (int i = 0; i < n; ++i) {
        const int cls = classes[i];
        ConvW c0, c1;
        int rc = stage_conv(c0, r.ops0, f16x3, w0[i], nullptr, b0[i], Cin, hid, 3, 3, feat, (size_t)B * HW * Cin, nullptr, 0, s);
        if (rc == CP_OK) rc = stage_conv(c1, r.ops1, false, w1[i], nullptr, b1[i], hid, cls, 1, 1, nullptr, 0, nullptr, 0, s);
        if (rc != CP_OK) return fail(rc, "pose_heads_forward: weight packing failed");
        for (int b = 0; b < B; b += chunk) {
            const int nb = std::min(chunk, B - b);
            const float* src = feat + (size_t)b * HW * Cin;
            ConvParams p = conv_params(nb, H, W, &src, &Cin, 1, c0, 1, 1, CP_ACT_RELU);
            p.out = r.hid;
            p.store = CP_STORE_NHWC;
            p.ldo = hid;
            rc = launch_conv(p, c0, r.ops0, f16x3, s);
            if (rc != CP_OK) return fail(rc, "pose_heads_forward: 3x3 launch failed");
            const float* hsrc = r.hid;
            ConvParams q = conv_params(nb, H, W, &hsrc, &hid, 1, c1, 1, 0, CP_ACT_NONE);
            q.out = out[i] + (size_t)b * cls * HW;
            q.store = CP_STORE_NCHW;
            q.ldo = cls;
            rc = cp_launch_conv(q, s);
            if (rc != CP_OK) return fail(rc, "pose_heads_forward: 1x1 launch failed");
        }
    }
    return CP_OK;
}

// The prediction heads' backward (heads_bwd.hip).  One implementation under two pairs of entry points: the plain pair is
// CP_PREC_F32; CP_PREC_F16X3 runs the three wide contractions of a head on the split-binary16 kernels.
static size_t pose_heads_backward_query(int B, int H, int W, int Cin, int hid, int n, const int* classes, int precision) {
    int cmax = 0;
    if (refused(heads_shape_error(B, H, W, Cin, hid, n, classes, &cmax), "pose_heads_backward", precision)) return 0;
    return cp_pose_heads_backward_ws_bytes(B, H, W, Cin, hid, cmax, precision);
}

static int pose_heads_backward_run(cp_stream_t stream, const float* feat, int n, const float* const* w0, const float* const* b0,
                                   const float* const* w1, const float* const* b1, const int* classes,
                                   const float* const* grad_out, float* const* grad_w0, float* const* grad_b0,
                                   float* const* grad_w1, float* const* grad_b1, float* grad_feat, int B, int H, int W, int Cin,
                                   int hid, int precision, void* workspace, size_t workspace_bytes) {
    int cmax = 0;
    if (refused(heads_shape_error(B, H, W, Cin, hid, n, classes, &cmax), "pose_heads_backward", precision)) return CP_ERR_INVALID;
    if (!feat || !w0 || !b0 || !w1 || !b1 || !grad_out || !grad_w0 || !grad_b0 || !grad_w1 || !grad_b1 || !workspace)
        return fail(CP_ERR_INVALID, "pose_heads_backward: null argument");
    for (int i = 0; i < n; ++i)
        if (!w0[i] || !b0[i] || !w1[i] || !b1[i] || !grad_w0[i] || !grad_b0[i] || !grad_w1[i] || !grad_b1[i])
            return fail(CP_ERR_INVALID, "pose_heads_backward: null argument");
    if (workspace_bytes < cp_pose_heads_backward_ws_bytes(B, H, W, Cin, hid, cmax, precision))
        return fail(CP_ERR_INVALID, "pose_heads_backward: workspace too small");
    const PoseHeadsArgs a{feat, n, w0, b0, w1, b1, classes, B, H, W, Cin, hid};
    const int rc = cp_launch_pose_heads_backward((hipStream_t)stream, a, grad_out, grad_w0, grad_b0, grad_w1, grad_b1, grad_feat,
                                                 workspace, precision);
    return rc == CP_OK ? CP_OK : fail(rc, "pose_heads_backward: kernel launch failed");
}

size_t cp_pose_heads_backward_workspace_bytes(int B, int H, int W, int Cin, int hid, int n, const int* classes) {
    return pose_heads_backward_query(B, H, W, Cin, hid, n, classes, CP_PREC_F32);
}

int cp_pose_heads_backward(cp_stream_t stream, const float* feat, int n, const float* const* w0, const float* const* b0,
                           const float* const* w1, const float* const* b1, const int* classes, const float* const* grad_out,
                           float* const* grad_w0, float* const* grad_b0, float* const* grad_w1, float* const* grad_b1,
                           float* grad_feat, int B, int H, int W, int Cin, int hid, void* workspace, size_t workspace_bytes) {
    return pose_heads_backward_run(stream, feat, n, w0, b0, w1, b1, classes, grad_out, grad_w0, grad_b0, grad_w1, grad_b1, grad_feat,
                                   B, H, W, Cin, hid, CP_PREC_F32, workspace, workspace_bytes);
}

size_t cp_pose_heads_backward_prec_workspace_bytes(int B, int H, int W, int Cin, int hid, int n, const int* classes, int precision) {
    return pose_heads_backward_query(B, H, W, Cin, hid, n, classes, precision);
}

int cp_pose_heads_backward_prec(cp_stream_t stream, const float* feat, int n, const float* const* w0, const float* const* b0,
                                const float* const* w1, const float* const* b1, const int* classes, const float* const* grad_out,
                                float* const* grad_w0, float* const* grad_b0, float* const* grad_w1, float* const* grad_b1,
                                float* grad_feat, int B, int H, int W, int Cin, int hid, int precision, void* workspace,
                                size_t workspace_bytes) {
    return pose_heads_backward_run(stream, feat, n, w0, b0, w1, b1, classes, grad_out, grad_w0, grad_b0, grad_w1, grad_b1, grad_feat,
                                   B, H, W, Cin, hid, precision, workspace, workspace_bytes);
}

// (which contractions run in f16x3 does not depend on the heads: the shape is checked as that of one single-class head)
int cp_pose_heads_backward_prec_mask(int B, int H, int W, int Cin, int hid, int precision) {
    const int one = 1;
    int cmax = 0;
    return refused(heads_shape_error(B, H, W, Cin, hid, 1, &one, &cmax), "pose_heads_backward", precision)
               ? CP_ERR_INVALID
               : cp_pose_heads_backward_mask(B, H, W, Cin, hid, precision);
}

size_t cp_conv2d_workspace_bytes(int Cin, int Cout, int KH, int KW) {
    Carve c{nullptr};
    conv2d_carve(c, Cin, Cout, KH, KW);
    return c.off;
}

size_t cp_conv_transpose2d_workspace_bytes(int Cin, int Cout) {
    Carve c{nullptr};
    deconv_carve(c, Cin, Cout);
    return c.off;
}

size_t cp_dcnv2_workspace_bytes(int B, int C, int H, int W, int Co) {
    Carve c{nullptr};
    dcn_carve(c, B, C, H, W, Co);
    return c.off;
}

int cp_conv_transpose2d_nhwc(cp_stream_t stream, const float* x, const float* w, const float* scale, const float* shift, float* out,
                             int B, int H, int W, int Cin, int Cout, int act, void* workspace, size_t workspace_bytes) {
    if (!x || !w || !out || !workspace) return fail(CP_ERR_INVALID, "conv_transpose2d_forward: null argument");
    if (B < 1 || H < 1 || W < 1 || Cout < 1) return fail(CP_ERR_INVALID, "conv_transpose2d_forward: empty shape");
    if (Cin % 32) return fail(CP_ERR_INVALID, "conv_transpose2d_forward: Cin must be a multiple of 32");
    if (act != CP_ACT_NONE && act != CP_ACT_RELU)
        return fail(CP_ERR_INVALID, "conv_transpose2d_forward: act must be 0 (none) or 1 (relu)");
    Carve c{(char*)workspace};
    const DeconvWs r = deconv_carve(c, Cin, Cout);
    if (workspace_bytes < c.off) return fail(CP_ERR_INVALID, "conv_transpose2d_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const bool f16x3 = g_default_precision == CP_PREC_F16X3;
    int rc = cp_launch_pack_deconv(w, f16x3 ? nullptr : r.wf, f16x3 ? r.hi : nullptr, f16x3 ? r.lo : nullptr, r.inv, Cin, Cout, s);
    if (rc == CP_OK && f16x3) {
        // range-safe operands as in cp_conv2d_nhwc: per-channel weight scale (folded into scale16), per-tensor activation scale
        if (hipMemsetAsync(r.slot, 0, kSlotBytes, s) != hipSuccess) rc = CP_ERR_LAUNCH;
        if (rc == CP_OK) rc = cp_launch_scale16(scale, r.inv, r.sc16, Cout, s);
        if (rc == CP_OK) rc = cp_launch_absmax(x, (size_t)B * H * W * Cin, r.slot, s);
    }
    if (rc != CP_OK) return fail(rc, "conv_transpose2d_forward: deconv weight packing failed");
    DeconvW d;
    d.wf = r.wf;
    d.hi = r.hi;
    d.lo = r.lo;
    d.scale = scale;
    d.scale16 = r.sc16;
    d.shift = shift;
    d.Cin = Cin;
    d.Cout = Cout;
    rc = cp_launch_deconv(deconv_launch(d, f16x3, x, f16x3 ? r.slot : nullptr, B, H, W, out, nullptr, act == CP_ACT_RELU), s);
    return rc == CP_OK ? CP_OK : fail(rc, "conv_transpose2d_forward: deconv launch failed (shape too large for 32-bit offsets?)");
}

int cp_conv2d_nhwc(cp_stream_t stream, const float* x, const float* w, const float* scale, const float* shift,
                   const float* residual, float* out, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                   int stride, int pad, int act, void* workspace, size_t workspace_bytes) {
    if (!x || !w || !out || !workspace) return fail(CP_ERR_INVALID, "conv2d_forward: null argument");
    if (Cin % 4) return fail(CP_ERR_INVALID, "conv2d_forward: Cin must be a multiple of 4");
    Carve c{(char*)workspace};
    const ConvOps r = conv2d_carve(c, Cin, Cout, KH, KW);
    if (workspace_bytes < c.off) return fail(CP_ERR_INVALID, "conv2d_forward: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const bool f16x3 = g_default_precision == CP_PREC_F16X3 && Cin % 32 == 0 && KH * KW <= 32 && cp_conv_tile_n(Cout) >= 32;
    ConvW cw;
    int rc = stage_conv(cw, r, f16x3, w, scale, shift, Cin, Cout, KH, KW, x, (size_t)B * H * W * Cin, nullptr, 0, s);
    if (rc != CP_OK) return fail(rc, "conv2d_forward: weight packing failed");
    ConvParams p = conv_params(B, H, W, &x, &Cin, 1, cw, stride, pad, act);
    // A ReLU of this entry keeps a NaN (cp_relu).  pw16.hip's epilogue keeps the inference engine's fmaxf -- its instruction stream
    // is pinned (tests/test_pooled_store_cpu.py) -- so a 1x1 layer that ends in a ReLU takes the LDS-staged loop here.
    if (act == CP_ACT_RELU) p.dbg |= CP_SEL_PW16_NEVER;
    p.res = residual;
    p.res_ld = Cout;
    p.out = out;
    p.store = CP_STORE_NHWC;
    p.ldo = Cout;
    rc = launch_conv(p, cw, r, f16x3, s);
    return rc == CP_OK ? CP_OK : fail(rc, "conv2d_forward: kernel launch failed");
}

int cp_conv2d_backward_path(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    if (const char* e = conv_bwd_shape_error(B, H, W, Cin, Cout, KH, KW, stride, pad)) return fail(CP_ERR_INVALID, e);
    return cp_conv_backward_path(B, H, W, Cin, Cout, KH, KW, stride, pad);
}

// The Conv2d backward (conv_bwd.hip).  One implementation under two pairs of entry points: the plain pair is CP_PREC_F32;
// CP_PREC_F16X3 runs the MFMA path's contractions on conv_bwd16.hip.
static size_t conv2d_backward_query(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int need_grad_x,
                                    int precision) {
    if (refused(conv_bwd_shape_error(B, H, W, Cin, Cout, KH, KW, stride, pad), "conv2d_backward", precision)) return 0;
    return cp_conv_backward_ws_bytes(B, H, W, Cin, Cout, KH, KW, stride, pad, need_grad_x, precision);
}

static int conv2d_backward_run(cp_stream_t stream, const float* x, const float* w, const float* y_or_null, const float* grad_out,
                               float* grad_x_or_null, float* grad_w, float* grad_bias_or_null, int B, int H, int W, int Cin,
                               int Cout, int KH, int KW, int stride, int pad, int precision, void* workspace,
                               size_t workspace_bytes) {
    if (refused(conv_bwd_shape_error(B, H, W, Cin, Cout, KH, KW, stride, pad), "conv2d_backward", precision)) return CP_ERR_INVALID;
    if (!x || !w || !grad_out || !grad_w || !workspace) return fail(CP_ERR_INVALID, "conv2d_backward: null argument");
    if (workspace_bytes < cp_conv_backward_ws_bytes(B, H, W, Cin, Cout, KH, KW, stride, pad, grad_x_or_null != nullptr, precision))
        return fail(CP_ERR_INVALID, "conv2d_backward: workspace too small");
    const ConvBwdArgs a{x, w, y_or_null, grad_out, grad_x_or_null, grad_w, grad_bias_or_null, B, H, W, Cin, Cout, KH, KW, stride, pad};
    const int rc = cp_launch_conv_backward((hipStream_t)stream, a, workspace, precision);
    return rc == CP_OK ? CP_OK : fail(rc, "conv2d_backward: kernel launch failed");
}

size_t cp_conv2d_backward_workspace_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                          int need_grad_x) {
    return conv2d_backward_query(B, H, W, Cin, Cout, KH, KW, stride, pad, need_grad_x, CP_PREC_F32);
}

int cp_conv2d_backward_nhwc(cp_stream_t stream, const float* x, const float* w, const float* y_or_null, const float* grad_out,
                            float* grad_x_or_null, float* grad_w, float* grad_bias_or_null, int B, int H, int W, int Cin,
                            int Cout, int KH, int KW, int stride, int pad, void* workspace, size_t workspace_bytes) {
    return conv2d_backward_run(stream, x, w, y_or_null, grad_out, grad_x_or_null, grad_w, grad_bias_or_null, B, H, W, Cin, Cout, KH,
                               KW, stride, pad, CP_PREC_F32, workspace, workspace_bytes);
}

size_t cp_conv2d_backward_prec_workspace_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                               int need_grad_x, int precision) {
    return conv2d_backward_query(B, H, W, Cin, Cout, KH, KW, stride, pad, need_grad_x, precision);
}

int cp_conv2d_backward_prec_nhwc(cp_stream_t stream, const float* x, const float* w, const float* y_or_null, const float* grad_out,
                                 float* grad_x_or_null, float* grad_w, float* grad_bias_or_null, int B, int H, int W, int Cin,
                                 int Cout, int KH, int KW, int stride, int pad, int precision, void* workspace,
                                 size_t workspace_bytes) {
    return conv2d_backward_run(stream, x, w, y_or_null, grad_out, grad_x_or_null, grad_w, grad_bias_or_null, B, H, W, Cin, Cout, KH,
                               KW, stride, pad, precision, workspace, workspace_bytes);
}

int cp_conv2d_backward_prec_mask(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int precision) {
    return refused(conv_bwd_shape_error(B, H, W, Cin, Cout, KH, KW, stride, pad), "conv2d_backward", precision)
               ? CP_ERR_INVALID
               : cp_conv_backward_prec_mask(B, H, W, Cin, Cout, KH, KW, stride, pad, precision);
}

int cp_conv_transpose2d_dw_nhwc(cp_stream_t stream, const float* x, const float* w, const float* add_or_null, float* out, int B,
                                int H, int W, int C, int f) {
    if (const char* e = deconv_shape_error(B, H, W, C, C, 2 * f, f, f / 2, C)) return fail(CP_ERR_INVALID, e);
    if (!x || !w || !out) return fail(CP_ERR_INVALID, "conv_transpose2d_dw: null argument");
    if (!bn_aligned({x, w, add_or_null, out})) return fail(CP_ERR_INVALID, "conv_transpose2d_dw: tensors must be 16-byte aligned");
    const int rc = cp_launch_upsample_add(x, w, add_or_null, out, B, H, W, C, f, nullptr, (hipStream_t)stream);
    return rc == CP_OK ? CP_OK : fail(rc, "conv_transpose2d_dw: kernel launch failed");
}

// The ConvTranspose2d backward (deconv_bwd.hip).  One implementation under two pairs of entry points: the plain pair is
// CP_PREC_F32; CP_PREC_F16X3 runs the dense layer's contractions on conv_bwd16.hip and igemm16.hip.
static size_t deconv_backward_query(int B, int H, int W, int Cin, int Cout, int K, int stride, int pad, int groups, int need_grad_x,
                                    int precision) {
    if (refused(deconv_shape_error(B, H, W, Cin, Cout, K, stride, pad, groups), "conv_transpose2d_backward", precision)) return 0;
    return cp_deconv_backward_ws_bytes(B, H, W, Cin, Cout, stride, groups, need_grad_x, precision);
}

static int deconv_backward_run(cp_stream_t stream, const float* x, const float* w, const float* grad_out, float* grad_x_or_null,
                               float* grad_w, int B, int H, int W, int Cin, int Cout, int K, int stride, int pad, int groups,
                               int precision, void* workspace, size_t workspace_bytes) {
    if (refused(deconv_shape_error(B, H, W, Cin, Cout, K, stride, pad, groups), "conv_transpose2d_backward", precision))
        return CP_ERR_INVALID;
    if (!x || !w || !grad_out || !grad_w || !workspace) return fail(CP_ERR_INVALID, "conv_transpose2d_backward: null argument");
    if (!bn_aligned({x, w, grad_out, grad_x_or_null, grad_w, workspace}))
        return fail(CP_ERR_INVALID, "conv_transpose2d_backward: tensors must be 16-byte aligned");
    if (workspace_bytes < cp_deconv_backward_ws_bytes(B, H, W, Cin, Cout, stride, groups, grad_x_or_null != nullptr, precision))
        return fail(CP_ERR_INVALID, "conv_transpose2d_backward: workspace too small");
    const DeconvBwdArgs a{x, w, grad_out, grad_x_or_null, grad_w, B, H, W, Cin, Cout, stride, groups};
    const int rc = cp_launch_deconv_backward((hipStream_t)stream, a, workspace, precision);
    return rc == CP_OK ? CP_OK : fail(rc, "conv_transpose2d_backward: kernel launch failed");
}

size_t cp_conv_transpose2d_backward_workspace_bytes(int B, int H, int W, int Cin, int Cout, int K, int stride, int pad, int groups,
                                                    int need_grad_x) {
    return deconv_backward_query(B, H, W, Cin, Cout, K, stride, pad, groups, need_grad_x, CP_PREC_F32);
}

int cp_conv_transpose2d_backward_nhwc(cp_stream_t stream, const float* x, const float* w, const float* grad_out,
                                      float* grad_x_or_null, float* grad_w, int B, int H, int W, int Cin, int Cout, int K,
                                      int stride, int pad, int groups, void* workspace, size_t workspace_bytes) {
    return deconv_backward_run(stream, x, w, grad_out, grad_x_or_null, grad_w, B, H, W, Cin, Cout, K, stride, pad, groups, CP_PREC_F32,
                               workspace, workspace_bytes);
}

size_t cp_conv_transpose2d_backward_prec_workspace_bytes(int B, int H, int W, int Cin, int Cout, int K, int stride, int pad,
                                                         int groups, int need_grad_x, int precision) {
    return deconv_backward_query(B, H, W, Cin, Cout, K, stride, pad, groups, need_grad_x, precision);
}

int cp_conv_transpose2d_backward_prec_nhwc(cp_stream_t stream, const float* x, const float* w, const float* grad_out,
                                           float* grad_x_or_null, float* grad_w, int B, int H, int W, int Cin, int Cout, int K,
                                           int stride, int pad, int groups, int precision, void* workspace,
                                           size_t workspace_bytes) {
    return deconv_backward_run(stream, x, w, grad_out, grad_x_or_null, grad_w, B, H, W, Cin, Cout, K, stride, pad, groups, precision,
                               workspace, workspace_bytes);
}

int cp_conv_transpose2d_backward_prec_mask(int B, int H, int W, int Cin, int Cout, int K, int stride, int pad, int groups,
                                           int precision) {
    return refused(deconv_shape_error(B, H, W, Cin, Cout, K, stride, pad, groups), "conv_transpose2d_backward", precision)
               ? CP_ERR_INVALID
               : cp_deconv_backward_prec_mask(B, H, W, Cin, Cout, groups, precision);
}

size_t cp_batchnorm_workspace_bytes(int B, int H, int W, int C) {
    if (const char* e = bn_shape_error(B, H, W, C)) {
        fail(CP_ERR_INVALID, e);
        return 0;
    }
    return cp_batchnorm_ws_bytes(B, H, W, C);
}

int cp_batchnorm_forward_nhwc(cp_stream_t stream, const float* x, const float* gamma_or_null, const float* beta_or_null,
                              const float* residual_or_null, float* running_mean_or_null, float* running_var_or_null, float* y,
                              float* save_mean, float* save_invstd, int B, int H, int W, int C, int training, float momentum,
                              float eps, int act, void* workspace, size_t workspace_bytes) {
    if (const char* e = bn_shape_error(B, H, W, C)) return fail(CP_ERR_INVALID, e);
    if (!x || !y || !save_mean || !save_invstd || !workspace) return fail(CP_ERR_INVALID, "batchnorm_forward: null argument");
    if (training && (long long)B * H * W < 2)
        return fail(CP_ERR_INVALID, "batchnorm_forward: training needs more than one value per channel (B*H*W >= 2)");
    if (!training && (!running_mean_or_null || !running_var_or_null))
        return fail(CP_ERR_INVALID, "batchnorm_forward: evaluation needs running_mean and running_var");
    if (act != 0 && act != 1) return fail(CP_ERR_INVALID, "batchnorm_forward: act must be 0 (none) or 1 (relu)");
    if (!(eps >= 0.f)) return fail(CP_ERR_INVALID, "batchnorm_forward: eps must not be negative");
    if (y == x) return fail(CP_ERR_INVALID, "batchnorm_forward: y must not alias x");
    if (!bn_aligned({x, gamma_or_null, beta_or_null, residual_or_null, y, save_mean, save_invstd, workspace}))
        return fail(CP_ERR_INVALID, "batchnorm_forward: tensors must be 16-byte aligned");
    if (workspace_bytes < cp_batchnorm_ws_bytes(B, H, W, C)) return fail(CP_ERR_INVALID, "batchnorm_forward: workspace too small");
    const BnFwdArgs a{x, gamma_or_null, beta_or_null, residual_or_null, running_mean_or_null, running_var_or_null, y, save_mean,
                      save_invstd, B, H, W, C, training != 0, momentum, eps, act};
    const int rc = cp_launch_batchnorm_forward((hipStream_t)stream, a, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "batchnorm_forward: kernel launch failed");
}

int cp_batchnorm_backward_nhwc(cp_stream_t stream, const float* x, const float* y_or_null, const float* grad_out,
                               const float* gamma_or_null, const float* save_mean, const float* save_invstd, float* grad_x_or_null,
                               float* grad_residual_or_null, float* grad_gamma_or_null, float* grad_beta_or_null, int B, int H,
                               int W, int C, int training, void* workspace, size_t workspace_bytes) {
    if (const char* e = bn_shape_error(B, H, W, C)) return fail(CP_ERR_INVALID, e);
    if (!x || !grad_out || !save_mean || !save_invstd || !workspace) return fail(CP_ERR_INVALID, "batchnorm_backward: null argument");
    if (training && (long long)B * H * W < 2)
        return fail(CP_ERR_INVALID, "batchnorm_backward: training needs more than one value per channel (B*H*W >= 2)");
    if (!bn_aligned({x, y_or_null, grad_out, gamma_or_null, save_mean, save_invstd, grad_x_or_null, grad_residual_or_null, workspace}))
        return fail(CP_ERR_INVALID, "batchnorm_backward: tensors must be 16-byte aligned");
    if (workspace_bytes < cp_batchnorm_ws_bytes(B, H, W, C)) return fail(CP_ERR_INVALID, "batchnorm_backward: workspace too small");
    const BnBwdArgs a{x, y_or_null, grad_out, gamma_or_null, save_mean, save_invstd, grad_x_or_null, grad_residual_or_null,
                      grad_gamma_or_null, grad_beta_or_null, B, H, W, C, training != 0};
    const int rc = cp_launch_batchnorm_backward((hipStream_t)stream, a, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "batchnorm_backward: kernel launch failed");
}

int cp_batchnorm_sync_record_floats(int C) {
    if (C < 4 || C > 4096 || C % 4) {
        fail(CP_ERR_INVALID, "batchnorm: C must be a multiple of 4 in 4..4096");
        return 0;
    }
    return cp_batchnorm_sync_rec_floats(C);
}

int cp_batchnorm_sync_stats_nhwc(cp_stream_t stream, const float* x, float* record, int B, int H, int W, int C, void* workspace,
                                 size_t workspace_bytes) {
    if (const char* e = bn_shape_error(B, H, W, C)) return fail(CP_ERR_INVALID, e);
    if (!x || !record || !workspace) return fail(CP_ERR_INVALID, "batchnorm_sync_stats: null argument");
    if (!bn_aligned({x, record, workspace})) return fail(CP_ERR_INVALID, "batchnorm_sync_stats: tensors must be 16-byte aligned");
    if (workspace_bytes < cp_batchnorm_ws_bytes(B, H, W, C)) return fail(CP_ERR_INVALID, "batchnorm_sync_stats: workspace too small");
    const int rc = cp_launch_batchnorm_sync_stats((hipStream_t)stream, x, record, B, H, W, C, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "batchnorm_sync_stats: kernel launch failed");
}

int cp_batchnorm_sync_forward_nhwc(cp_stream_t stream, const float* x, const float* gamma_or_null, const float* beta_or_null,
                                   const float* residual_or_null, float* running_mean_or_null, float* running_var_or_null, float* y,
                                   float* save_mean, float* save_invstd, float* save_count, const float* records, int world, int B,
                                   int H, int W, int C, float momentum, float eps, int act, void* workspace,
                                   size_t workspace_bytes) {
    if (const char* e = bn_shape_error(B, H, W, C)) return fail(CP_ERR_INVALID, e);
    if (!x || !y || !save_mean || !save_invstd || !save_count || !records || !workspace)
        return fail(CP_ERR_INVALID, "batchnorm_sync_forward: null argument");
    if (world < 1 || world > 1024) return fail(CP_ERR_INVALID, "batchnorm_sync_forward: world must be in 1..1024");
    // (every rank holds at least one value per channel, so only a single rank can fall short of two)
    if (world == 1 && (long long)B * H * W < 2)
        return fail(CP_ERR_INVALID, "batchnorm_sync_forward: needs more than one value per channel over the ranks (global count >= 2)");
    if (act != 0 && act != 1) return fail(CP_ERR_INVALID, "batchnorm_sync_forward: act must be 0 (none) or 1 (relu)");
    if (!(eps >= 0.f)) return fail(CP_ERR_INVALID, "batchnorm_sync_forward: eps must not be negative");
    if (y == x) return fail(CP_ERR_INVALID, "batchnorm_sync_forward: y must not alias x");
    if (!bn_aligned({x, gamma_or_null, beta_or_null, residual_or_null, y, save_mean, save_invstd, records, workspace}))
        return fail(CP_ERR_INVALID, "batchnorm_sync_forward: tensors must be 16-byte aligned");
    if (workspace_bytes < cp_batchnorm_ws_bytes(B, H, W, C)) return fail(CP_ERR_INVALID, "batchnorm_sync_forward: workspace too small");
    const BnFwdArgs a{x, gamma_or_null, beta_or_null, residual_or_null, running_mean_or_null, running_var_or_null, y, save_mean,
                      save_invstd, B, H, W, C, 1, momentum, eps, act};
    const int rc = cp_launch_batchnorm_sync_forward((hipStream_t)stream, a, records, world, save_count);
    return rc == CP_OK ? CP_OK : fail(rc, "batchnorm_sync_forward: kernel launch failed");
}

int cp_batchnorm_sync_backward_reduce_nhwc(cp_stream_t stream, const float* x, const float* y_or_null, const float* grad_out,
                                           const float* save_mean, const float* save_invstd, float* sums, float* grad_gamma_or_null,
                                           float* grad_beta_or_null, int B, int H, int W, int C, void* workspace,
                                           size_t workspace_bytes) {
    if (const char* e = bn_shape_error(B, H, W, C)) return fail(CP_ERR_INVALID, e);
    if (!x || !grad_out || !save_mean || !save_invstd || !sums || !workspace)
        return fail(CP_ERR_INVALID, "batchnorm_sync_backward_reduce: null argument");
    if (!bn_aligned({x, y_or_null, grad_out, save_mean, save_invstd, sums, workspace}))
        return fail(CP_ERR_INVALID, "batchnorm_sync_backward_reduce: tensors must be 16-byte aligned");
    if (workspace_bytes < cp_batchnorm_ws_bytes(B, H, W, C))
        return fail(CP_ERR_INVALID, "batchnorm_sync_backward_reduce: workspace too small");
    const BnBwdArgs a{x, y_or_null, grad_out, nullptr, save_mean, save_invstd, nullptr, nullptr, grad_gamma_or_null,
                      grad_beta_or_null, B, H, W, C, 1};
    const int rc = cp_launch_batchnorm_sync_backward_reduce((hipStream_t)stream, a, sums, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "batchnorm_sync_backward_reduce: kernel launch failed");
}

int cp_batchnorm_sync_backward_apply_nhwc(cp_stream_t stream, const float* x, const float* y_or_null, const float* grad_out,
                                          const float* gamma_or_null, const float* save_mean, const float* save_invstd,
                                          const float* sums_all, int world, const float* save_count, float* grad_x_or_null,
                                          float* grad_residual_or_null, int B, int H, int W, int C, void* workspace,
                                          size_t workspace_bytes) {
    if (const char* e = bn_shape_error(B, H, W, C)) return fail(CP_ERR_INVALID, e);
    if (!x || !grad_out || !save_mean || !save_invstd || !sums_all || !save_count || !workspace)
        return fail(CP_ERR_INVALID, "batchnorm_sync_backward_apply: null argument");
    if (world < 1 || world > 1024) return fail(CP_ERR_INVALID, "batchnorm_sync_backward_apply: world must be in 1..1024");
    if (!bn_aligned({x, y_or_null, grad_out, gamma_or_null, save_mean, save_invstd, sums_all, grad_x_or_null, grad_residual_or_null,
                     workspace}))
        return fail(CP_ERR_INVALID, "batchnorm_sync_backward_apply: tensors must be 16-byte aligned");
    if (workspace_bytes < cp_batchnorm_ws_bytes(B, H, W, C))
        return fail(CP_ERR_INVALID, "batchnorm_sync_backward_apply: workspace too small");
    if (!grad_x_or_null && !grad_residual_or_null) return CP_OK;
    const BnBwdArgs a{x, y_or_null, grad_out, gamma_or_null, save_mean, save_invstd, grad_x_or_null, grad_residual_or_null,
                      nullptr, nullptr, B, H, W, C, 1};
    const int rc = cp_launch_batchnorm_sync_backward_apply((hipStream_t)stream, a, sums_all, world, save_count, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "batchnorm_sync_backward_apply: kernel launch failed");
}

size_t cp_groupnorm_workspace_bytes(int B, int H, int W, int C, int G) {
    if (const char* e = gn_shape_error(B, H, W, C, G)) {
        fail(CP_ERR_INVALID, e);
        return 0;
    }
    return cp_groupnorm_ws_bytes(B, H, W, C, G);
}

int cp_groupnorm_forward_nhwc(cp_stream_t stream, const float* x, const float* gamma_or_null, const float* beta_or_null, float* y,
                              float* save_mean, float* save_invstd, int B, int H, int W, int C, int G, float eps, int act,
                              void* workspace, size_t workspace_bytes) {
    if (const char* e = gn_shape_error(B, H, W, C, G)) return fail(CP_ERR_INVALID, e);
    if (!x || !y || !save_mean || !save_invstd || !workspace) return fail(CP_ERR_INVALID, "groupnorm_forward: null argument");
    if (act != 0 && act != 1) return fail(CP_ERR_INVALID, "groupnorm_forward: act must be 0 (none) or 1 (relu)");
    if (!(eps >= 0.f)) return fail(CP_ERR_INVALID, "groupnorm_forward: eps must not be negative");
    if (y == x) return fail(CP_ERR_INVALID, "groupnorm_forward: y must not alias x");
    if (!bn_aligned({x, gamma_or_null, beta_or_null, y, save_mean, save_invstd, workspace}))
        return fail(CP_ERR_INVALID, "groupnorm_forward: tensors must be 16-byte aligned");
    if (workspace_bytes < cp_groupnorm_ws_bytes(B, H, W, C, G)) return fail(CP_ERR_INVALID, "groupnorm_forward: workspace too small");
    const GnFwdArgs a{x, gamma_or_null, beta_or_null, y, save_mean, save_invstd, B, H, W, C, G, eps, act};
    const int rc = cp_launch_groupnorm_forward((hipStream_t)stream, a, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "groupnorm_forward: kernel launch failed");
}

int cp_groupnorm_backward_nhwc(cp_stream_t stream, const float* x, const float* y_or_null, const float* grad_out,
                               const float* gamma_or_null, const float* save_mean, const float* save_invstd, float* grad_x_or_null,
                               float* grad_gamma_or_null, float* grad_beta_or_null, int B, int H, int W, int C, int G,
                               void* workspace, size_t workspace_bytes) {
    if (const char* e = gn_shape_error(B, H, W, C, G)) return fail(CP_ERR_INVALID, e);
    if (!x || !grad_out || !save_mean || !save_invstd || !workspace) return fail(CP_ERR_INVALID, "groupnorm_backward: null argument");
    if (!bn_aligned({x, y_or_null, grad_out, gamma_or_null, save_mean, save_invstd, grad_x_or_null, grad_gamma_or_null,
                     grad_beta_or_null, workspace}))
        return fail(CP_ERR_INVALID, "groupnorm_backward: tensors must be 16-byte aligned");
    if (workspace_bytes < cp_groupnorm_ws_bytes(B, H, W, C, G)) return fail(CP_ERR_INVALID, "groupnorm_backward: workspace too small");
    const GnBwdArgs a{x, y_or_null, grad_out, gamma_or_null, save_mean, save_invstd, grad_x_or_null, grad_gamma_or_null,
                      grad_beta_or_null, B, H, W, C, G};
    const int rc = cp_launch_groupnorm_backward((hipStream_t)stream, a, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "groupnorm_backward: kernel launch failed");
}

// The ConvGRU's gate arithmetic (gru_train.hip)
int cp_gru_gate_forward(cp_stream_t stream, const float* x3, const float* h3_or_null, const float* hprev_or_null, float* hout, int M,
                        int Ch) {
    if (const char* e = gru_shape_error(M, Ch)) return fail(CP_ERR_INVALID, e);
    if (!x3 || !hout) return fail(CP_ERR_INVALID, "gru_gate_forward: null argument");
    if (!h3_or_null != !hprev_or_null)
        return fail(CP_ERR_INVALID, "gru_gate_forward: h3 and hprev are given together, or neither (step 0: h = 0)");
    if (!bn_aligned({x3, h3_or_null, hprev_or_null, hout})) return fail(CP_ERR_INVALID, "gru_gate_forward: tensors must be 16-byte aligned");
    const int rc = cp_launch_gru_gate_forward((hipStream_t)stream, x3, h3_or_null, hprev_or_null, hout, M, Ch);
    return rc == CP_OK ? CP_OK : fail(rc, "gru_gate_forward: kernel launch failed");
}

int cp_gru_gate_backward(cp_stream_t stream, const float* x3, const float* h3_or_null, const float* hprev_or_null,
                         const float* grad_hout, float* grad_x3, float* grad_h3_or_null, float* grad_hprev_or_null, int M, int Ch) {
    if (const char* e = gru_shape_error(M, Ch)) return fail(CP_ERR_INVALID, e);
    if (!x3 || !grad_hout || !grad_x3) return fail(CP_ERR_INVALID, "gru_gate_backward: null argument");
    if (!h3_or_null != !hprev_or_null)
        return fail(CP_ERR_INVALID, "gru_gate_backward: h3 and hprev are given together, or neither (step 0: h = 0)");
    if (!h3_or_null && (grad_h3_or_null || grad_hprev_or_null))
        return fail(CP_ERR_INVALID, "gru_gate_backward: step 0 (h3 == NULL) has no hidden-side gradients");
    if (!bn_aligned({x3, h3_or_null, hprev_or_null, grad_hout, grad_x3, grad_h3_or_null, grad_hprev_or_null}))
        return fail(CP_ERR_INVALID, "gru_gate_backward: tensors must be 16-byte aligned");
    const int rc = cp_launch_gru_gate_backward((hipStream_t)stream, x3, h3_or_null, hprev_or_null, grad_hout, grad_x3, grad_h3_or_null,
                                               grad_hprev_or_null, M, Ch);
    return rc == CP_OK ? CP_OK : fail(rc, "gru_gate_backward: kernel launch failed");
}

// MaxPool2d, forward and backward (pool.hip)
static const char* maxpool_shape_error(int B, int H, int W, int C, int kernel, int stride, int pad) {
    if (!cp_maxpool_geometry(kernel, stride, pad))
        return "maxpool2d: unsupported geometry ((kernel, stride, padding) must be (2, 2, 0) or (3, 2, 1))";
    if (B < 1 || H < 1 || W < 1) return "maxpool2d: B, H and W must be at least 1";
    if (C < 4 || C % 4) return "maxpool2d: C must be a positive multiple of 4";
    if (H + 2 * pad < kernel || W + 2 * pad < kernel) return "maxpool2d: empty output (the window is larger than the padded input)";
    if ((long long)B * H * W * C >= 0x7fffffffLL) return "maxpool2d: a tensor has 2^31 elements or more";
    return nullptr;
}

int cp_maxpool2d_forward_nhwc(cp_stream_t stream, const float* x, float* out, int B, int H, int W, int C, int kernel, int stride,
                              int pad) {
    if (const char* e = maxpool_shape_error(B, H, W, C, kernel, stride, pad)) return fail(CP_ERR_INVALID, e);
    if (!x || !out) return fail(CP_ERR_INVALID, "maxpool2d_forward: null argument");
    if (!bn_aligned({x, out})) return fail(CP_ERR_INVALID, "maxpool2d_forward: tensors must be 16-byte aligned");
    const int rc = cp_launch_maxpool_forward((hipStream_t)stream, x, out, B, H, W, C, kernel);
    return rc == CP_OK ? CP_OK : fail(rc, "maxpool2d_forward: kernel launch failed");
}

int cp_maxpool2d_backward_nhwc(cp_stream_t stream, const float* x, const float* grad_out, float* grad_x, int B, int H, int W, int C,
                               int kernel, int stride, int pad) {
    if (const char* e = maxpool_shape_error(B, H, W, C, kernel, stride, pad)) return fail(CP_ERR_INVALID, e);
    if (!x || !grad_out || !grad_x) return fail(CP_ERR_INVALID, "maxpool2d_backward: null argument");
    if (!bn_aligned({x, grad_out, grad_x})) return fail(CP_ERR_INVALID, "maxpool2d_backward: tensors must be 16-byte aligned");
    const int rc = cp_launch_maxpool_backward((hipStream_t)stream, x, grad_out, grad_x, B, H, W, C, kernel);
    return rc == CP_OK ? CP_OK : fail(rc, "maxpool2d_backward: kernel launch failed");
}

// The hourglass merge up1 + nearest2x(low), forward and backward (ewise.hip)
static const char* upsample2_shape_error(int B, int H, int W, int C) {
    if (B < 1 || H < 1 || W < 1) return "upsample2_add: B, H and W must be at least 1";
    if (C < 4 || C % 4) return "upsample2_add: C must be a positive multiple of 4";
    const long long lim = 0x7fffffffLL;  // of the [B,2H,2W,C] tensors; every partial product below stays under 2^62
    long long n = 4LL * B;
    if (n >= lim || (n *= H) >= lim || (n *= W) >= lim || (n *= C) >= lim) return "upsample2_add: a tensor has 2^31 elements or more";
    return nullptr;
}

int cp_upsample2_add_nhwc(cp_stream_t stream, const float* up1, const float* low, float* out, int B, int H, int W, int C) {
    if (const char* e = upsample2_shape_error(B, H, W, C)) return fail(CP_ERR_INVALID, e);
    if (!up1 || !low || !out) return fail(CP_ERR_INVALID, "upsample2_add: null argument");
    if (!bn_aligned({up1, low, out})) return fail(CP_ERR_INVALID, "upsample2_add: tensors must be 16-byte aligned");
    const int rc = cp_launch_upsample2_nearest_add(up1, low, out, B, H, W, C, nullptr, (hipStream_t)stream);
    return rc == CP_OK ? CP_OK : fail(rc, "upsample2_add: kernel launch failed");
}

int cp_upsample2_add_backward_nhwc(cp_stream_t stream, const float* grad_out, float* grad_low, int B, int H, int W, int C) {
    if (const char* e = upsample2_shape_error(B, H, W, C)) return fail(CP_ERR_INVALID, e);
    if (!grad_out || !grad_low) return fail(CP_ERR_INVALID, "upsample2_add_backward: null argument");
    if (!bn_aligned({grad_out, grad_low})) return fail(CP_ERR_INVALID, "upsample2_add_backward: tensors must be 16-byte aligned");
    const int rc = cp_launch_upsample2_nearest_add_backward(grad_out, grad_low, B, H, W, C, (hipStream_t)stream);
    return rc == CP_OK ? CP_OK : fail(rc, "upsample2_add_backward: kernel launch failed");
}

// The image stems' weight / bias gradient (stem_bwd.hip)
// Two pairs of entry points over one launcher: the narrow pair keeps its range (Cout up to 64), the wide pair takes Cout up
// to 128, the hourglass's stem, which the launcher splits into channel blocks
static size_t stem_backward_query(bool wide, int B, int H, int W, int Cin, int Cout, int stride) {
    if (const char* e = cp_stem_backward_shape_error(B, H, W, Cin, Cout, stride, wide)) {
        fail(CP_ERR_INVALID, e);
        return 0;
    }
    return cp_stem_backward_ws_bytes(B, H, W, Cin, Cout, stride);
}

static int stem_backward_run(bool wide, cp_stream_t stream, const float* x_nchw, const float* grad_out_nhwc, const float* y_or_null,
                             float* grad_w, float* grad_bias_or_null, void* workspace, size_t workspace_bytes, int B, int H, int W,
                             int Cin, int Cout, int stride) {
    if (const char* e = cp_stem_backward_shape_error(B, H, W, Cin, Cout, stride, wide)) return fail(CP_ERR_INVALID, e);
    if (!x_nchw || !grad_out_nhwc || !grad_w || !workspace) return fail(CP_ERR_INVALID, "conv2d_stem_backward: null argument");
    if (workspace_bytes < cp_stem_backward_ws_bytes(B, H, W, Cin, Cout, stride))
        return fail(CP_ERR_INVALID, "conv2d_stem_backward: workspace too small");
    const StemBwdArgs a{x_nchw, grad_out_nhwc, y_or_null, grad_w, grad_bias_or_null, B, H, W, Cin, Cout, stride};
    const int rc = cp_launch_stem_backward((hipStream_t)stream, a, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "conv2d_stem_backward: kernel launch failed");
}

size_t cp_conv2d_stem_backward_workspace_bytes(int B, int H, int W, int Cin, int Cout, int stride) {
    return stem_backward_query(false, B, H, W, Cin, Cout, stride);
}

int cp_conv2d_stem_backward(cp_stream_t stream, const float* x_nchw, const float* grad_out_nhwc, const float* y_or_null,
                            float* grad_w, float* grad_bias_or_null, void* workspace, size_t workspace_bytes, int B, int H, int W,
                            int Cin, int Cout, int stride) {
    return stem_backward_run(false, stream, x_nchw, grad_out_nhwc, y_or_null, grad_w, grad_bias_or_null, workspace, workspace_bytes,
                             B, H, W, Cin, Cout, stride);
}

size_t cp_conv2d_stem_wide_backward_workspace_bytes(int B, int H, int W, int Cin, int Cout, int stride) {
    return stem_backward_query(true, B, H, W, Cin, Cout, stride);
}

int cp_conv2d_stem_wide_backward(cp_stream_t stream, const float* x_nchw, const float* grad_out_nhwc, const float* y_or_null,
                                 float* grad_w, float* grad_bias_or_null, void* workspace, size_t workspace_bytes, int B, int H,
                                 int W, int Cin, int Cout, int stride) {
    return stem_backward_run(true, stream, x_nchw, grad_out_nhwc, y_or_null, grad_w, grad_bias_or_null, workspace, workspace_bytes,
                             B, H, W, Cin, Cout, stride);
}

// The DCNv2 backward (dcn_bwd.hip).  One implementation under three pairs of entry points: the plain pair (float atomics in
// grad_input) and the _det pair (bit-reproducible, the fast geometry only) are CP_PREC_F32; the _prec pair takes `deterministic`
// and the precision as arguments, CP_PREC_F16X3 running the fast geometry's contractions on dcn_bwd16.hip.
// The deterministic form refuses what the plain form refuses, and any geometry outside the fast path:
static std::string dcn_bwd_det_geometry_error(int C, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int dg) {
    if (cp_dcn_backward_fast(C, kh, kw, sh, sw, ph, pw, dh, dw, dg)) return std::string();
    char msg[320];
    snprintf(msg, sizeof msg,
             "dcn_v2_backward_det: geometry %dx%d / stride %d,%d / pad %d,%d / dilation %d,%d / deformable_group %d / C = %d is "
             "outside the deterministic path, which covers 3x3 / stride 1 / pad 1 / dilation 1 / one group / C %% 16 == 0",
             kh, kw, sh, sw, ph, pw, dh, dw, dg, C);
    return msg;
}

// What the call and the mask refuse before they look at anything else, recorded in cp_last_error: the shape (on success Ho,
// Wo are the output's), then the precision, then (deterministic only) the geometry
static bool dcn_backward_refused(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                 int dg, int deterministic, int precision, int* Ho, int* Wo) {
    if (refused(dcn_bwd_shape_error(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg, Ho, Wo), "dcn_v2_backward", precision)) return true;
    const std::string ge = deterministic ? dcn_bwd_det_geometry_error(C, kh, kw, sh, sw, ph, pw, dh, dw, dg) : std::string();
    if (!ge.empty()) fail(CP_ERR_INVALID, ge);
    return !ge.empty();
}

// The same checks in the same order, but a refused shape or geometry is 0 without a cp_last_error text, as these queries
// have answered since before there was a precision to name: only an unknown precision records one.
static size_t dcn_backward_query(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                 int dg, int deterministic, int precision) {
    int Ho = 0, Wo = 0;
    if (dcn_bwd_shape_error(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg, &Ho, &Wo)) return 0;
    if (refused(nullptr, "dcn_v2_backward", precision)) return 0;
    if (!deterministic) return cp_dcn_backward_ws_bytes(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, dg, precision);
    if (!cp_dcn_backward_fast(C, kh, kw, sh, sw, ph, pw, dh, dw, dg)) return 0;
    return cp_dcn_backward_det_ws_bytes(B, C, H, W, Co, precision);
}

static int dcn_backward_run(cp_stream_t stream, const float* input, const float* weight, const float* offset, const float* mask,
                            const float* grad_output, float* grad_input, float* grad_offset, float* grad_mask, float* grad_weight,
                            float* grad_bias, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                            int dh, int dw, int deformable_group, int deterministic, int precision, void* workspace,
                            size_t workspace_bytes) {
    int Ho = 0, Wo = 0;
    if (dcn_backward_refused(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, deterministic, precision, &Ho, &Wo))
        return CP_ERR_INVALID;
    const char* name = deterministic ? "dcn_v2_backward_det" : "dcn_v2_backward";
    if (!input || !weight || !offset || !mask || !grad_output || !grad_input || !grad_offset || !grad_mask || !grad_weight ||
        !grad_bias || !workspace)
        return fail(CP_ERR_INVALID, std::string(name) + ": null argument");
    const size_t need = deterministic ? cp_dcn_backward_det_ws_bytes(B, C, H, W, Co, precision)
                                      : cp_dcn_backward_ws_bytes(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, precision);
    if (workspace_bytes < need) return fail(CP_ERR_INVALID, std::string(name) + ": workspace too small");
    DcnBwdArgs a{input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight, grad_bias,
                 B, C, H, W, Co, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group};
    const int rc = deterministic ? cp_launch_dcn_backward_det((hipStream_t)stream, a, workspace, precision)
                                 : cp_launch_dcn_backward((hipStream_t)stream, a, workspace, precision);
    return rc == CP_OK ? CP_OK : fail(rc, std::string(name) + ": kernel launch failed");
}

size_t cp_dcnv2_backward_workspace_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                                         int dh, int dw, int deformable_group) {
    return dcn_backward_query(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, 0, CP_PREC_F32);
}

int cp_dcnv2_backward(cp_stream_t stream, const float* input, const float* weight, const float* offset, const float* mask,
                      const float* grad_output, float* grad_input, float* grad_offset, float* grad_mask, float* grad_weight,
                      float* grad_bias, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                      int dh, int dw, int deformable_group, void* workspace, size_t workspace_bytes) {
    return dcn_backward_run(stream, input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight,
                            grad_bias, B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, 0, CP_PREC_F32, workspace,
                            workspace_bytes);
}

size_t cp_dcnv2_backward_det_workspace_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                                             int dh, int dw, int deformable_group) {
    return dcn_backward_query(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, 1, CP_PREC_F32);
}

int cp_dcnv2_backward_det(cp_stream_t stream, const float* input, const float* weight, const float* offset, const float* mask,
                          const float* grad_output, float* grad_input, float* grad_offset, float* grad_mask, float* grad_weight,
                          float* grad_bias, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                          int dh, int dw, int deformable_group, void* workspace, size_t workspace_bytes) {
    return dcn_backward_run(stream, input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight,
                            grad_bias, B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, 1, CP_PREC_F32, workspace,
                            workspace_bytes);
}

size_t cp_dcnv2_backward_prec_workspace_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                                              int dh, int dw, int deformable_group, int deterministic, int precision) {
    return dcn_backward_query(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, deterministic, precision);
}

int cp_dcnv2_backward_prec(cp_stream_t stream, const float* input, const float* weight, const float* offset, const float* mask,
                           const float* grad_output, float* grad_input, float* grad_offset, float* grad_mask, float* grad_weight,
                           float* grad_bias, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw,
                           int dh, int dw, int deformable_group, int deterministic, int precision, void* workspace,
                           size_t workspace_bytes) {
    return dcn_backward_run(stream, input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight,
                            grad_bias, B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, deterministic, precision,
                            workspace, workspace_bytes);
}

int cp_dcnv2_backward_prec_mask(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                                int deformable_group, int deterministic, int precision) {
    int Ho = 0, Wo = 0;
    return dcn_backward_refused(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, deterministic, precision, &Ho, &Wo)
               ? CP_ERR_INVALID
               : cp_dcn_backward_prec_mask(B, C, H, W, Co, kh, kw, sh, sw, ph, pw, dh, dw, deformable_group, precision);
}

// DCNv2 forward with the reference's NCHW layouts (see header)
int cp_dcnv2_forward(cp_stream_t stream, const float* input, const float* weight, const float* bias, const float* offset,
                     const float* mask, float* output, int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw,
                     int ph, int pw, int dh, int dw, int deformable_group, void* workspace, size_t workspace_bytes) {
    if (!input || !weight || !bias || !offset || !mask || !output || !workspace)
        return fail(CP_ERR_INVALID, "dcn_v2_forward: null argument");
    if (B < 1 || C < 1 || H < 1 || W < 1 || Co < 1 || kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 || dh < 1 ||
        dw < 1 || deformable_group < 1 || C % deformable_group != 0)
        return fail(CP_ERR_INVALID, "dcn_v2_forward: bad shape argument (C must be divisible by deformable_group)");
    hipStream_t s = (hipStream_t)stream;
    const bool fast = kh == 3 && kw == 3 && sh == 1 && sw == 1 && ph == 1 && pw == 1 && dh == 1 && dw == 1 &&
                      deformable_group == 1 && C % 16 == 0 && cp_conv_tile_n(Co) >= 64 && !(g_dbg & CP_SEL_DCN_GENERIC);
    if (!fast) {
        // everything CenterPose does not use (other kernels / strides / dilations, deformable groups, tiny channel
        // counts): the generic float32 kernel on the reference's own layouts, no workspace
        const int Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1, Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
        if (Ho < 1 || Wo < 1) return fail(CP_ERR_INVALID, "dcn_v2_forward: empty output");
        const int rc = cp_launch_dcn_generic(s, input, weight, bias, offset, mask, output, B, C, H, W, Co, Ho, Wo, kh, kw, sh,
                                             sw, ph, pw, dh, dw, deformable_group);
        return rc == CP_OK ? CP_OK : fail(rc, "dcn_v2_forward: generic kernel launch failed");
    }
    Carve c{(char*)workspace};
    const DcnWs r = dcn_carve(c, B, C, H, W, Co);
    if (workspace_bytes < c.off) return fail(CP_ERR_INVALID, "dcn_v2_forward: workspace too small");
    const size_t px = (size_t)B * H * W;
    int rc = cp_launch_nchw_to_nhwc(input, r.x, B, C, H, W, C, s);
    if (rc != CP_OK) return fail(rc, "dcn_v2_forward: input re-layout failed");
    hipLaunchKernelGGL(dcn_offmask_pack_kernel, dim3(2048), dim3(256), 0, s, offset, mask, r.om, B, H * W);
    const bool f16x3 = g_default_precision == CP_PREC_F16X3 && C % 32 == 0;
    ConvW cw;
    rc = stage_conv(cw, r.ops, f16x3, weight, nullptr, bias, C, Co, 3, 3, r.x, px * C, r.om, px, s);
    if (rc != CP_OK) return fail(rc, "dcn_v2_forward: weight packing failed");
    const float* src = r.x;
    ConvParams p = conv_params(B, H, W, &src, &C, 1, cw, 1, 1, CP_ACT_NONE);
    p.out = r.y;
    p.store = CP_STORE_NHWC;
    p.ldo = Co;
    p.offmask = r.om;
    rc = launch_conv(p, cw, r.ops, f16x3, s);
    if (rc == CP_OK) rc = cp_launch_nhwc_to_nchw(r.y, output, B, Co, H, W, Co, s);
    return rc == CP_OK ? CP_OK : fail(rc, "dcn_v2_forward: kernel launch failed");
}

// Clip + Adam over a param group (optim.hip)
size_t cp_adam_table_bytes(int n_tensors, const int64_t* lengths, const int* active_or_null, int* n_chunks) {
    long long nc = 0;
    const char* e = cp_adam_lengths_check(n_tensors, lengths, active_or_null, &nc);
    if (!e && !n_chunks) e = "adam: null n_chunks";
    if (e) {
        fail(CP_ERR_INVALID, e);
        return 0;
    }
    *n_chunks = (int)nc;  // at most 2^31 / CP_ADAM_CHUNK + n_tensors
    return cp_adam_table_size(n_tensors, nc);
}

int cp_adam_table_build(void* table, size_t table_bytes, int n_tensors, const void* const* p, const void* const* g,
                        const void* const* m, const void* const* v, const int64_t* lengths, const int* active_or_null,
                        int* n_chunks) {
    if (!table || !p || !g || !m || !v || !lengths || !n_chunks) return fail(CP_ERR_INVALID, "adam_table_build: null argument");
    long long nc = 0;
    if (const char* e = cp_adam_lengths_check(n_tensors, lengths, active_or_null, &nc)) return fail(CP_ERR_INVALID, e);
    if (table_bytes < cp_adam_table_size(n_tensors, nc)) return fail(CP_ERR_INVALID, "adam_table_build: table buffer too small");
    if ((uintptr_t)table & 7) return fail(CP_ERR_INVALID, "adam_table_build: table must be 8-byte aligned");
    if (const char* e = cp_adam_table_fill(table, n_tensors, p, g, m, v, lengths, active_or_null)) return fail(CP_ERR_INVALID, e);
    *n_chunks = (int)nc;
    return CP_OK;
}

size_t cp_adam_state_bytes(int n_tensors) { return n_tensors < 1 ? 0 : CP_ADAM_STATE_BC(n_tensors) + (size_t)n_tensors * 16; }

size_t cp_adam_workspace_bytes(int n_chunks) { return n_chunks < 0 ? 0 : cp_adam_ws_bytes(n_chunks); }

int cp_adam_step(cp_stream_t stream, const void* table, int n_tensors, int n_chunks, double lr, double beta1, double beta2, double eps,
                 double weight_decay, double max_norm, int flags, void* state, void* workspace, size_t workspace_bytes) {
    if (!table || !state || !workspace) return fail(CP_ERR_INVALID, "adam_step: null argument");
    if (n_tensors < 1) return fail(CP_ERR_INVALID, "adam_step: n_tensors must be >= 1");
    if (n_chunks < 0) return fail(CP_ERR_INVALID, "adam_step: n_chunks must be >= 0");
    if (((uintptr_t)table | (uintptr_t)state | (uintptr_t)workspace) & 7)
        return fail(CP_ERR_INVALID, "adam_step: table, state and workspace must be 8-byte aligned");
    for (double h : {lr, beta1, beta2, eps, weight_decay, max_norm})
        if (!std::isfinite(h)) return fail(CP_ERR_INVALID, "adam_step: non-finite hyper-parameter");
    if (lr < 0) return fail(CP_ERR_INVALID, "adam_step: lr must be >= 0");
    if (!(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1)) return fail(CP_ERR_INVALID, "adam_step: betas must lie in [0, 1)");
    if (eps < 0) return fail(CP_ERR_INVALID, "adam_step: eps must be >= 0");
    if (weight_decay < 0) return fail(CP_ERR_INVALID, "adam_step: weight_decay must be >= 0");
    if (flags & ~CP_ADAM_SKIP_NONFINITE) return fail(CP_ERR_INVALID, "adam_step: unknown flag");
    if (workspace_bytes < cp_adam_ws_bytes(n_chunks)) return fail(CP_ERR_INVALID, "adam_step: workspace too small");
    const int rc = cp_launch_adam_step((hipStream_t)stream, table, n_tensors, n_chunks, lr, beta1, beta2, eps, weight_decay, max_norm,
                                       flags, state, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "adam_step: kernel launch failed");
}

// The gradient pack of data-parallel training (grad_pack.hip)
size_t cp_grad_flat_elems(int n_tensors, const int64_t* lengths) {
    long long total = 0;
    if (const char* e = cp_grad_layout(n_tensors, lengths, nullptr, &total, nullptr)) {
        fail(CP_ERR_INVALID, e);
        return 0;
    }
    return (size_t)total;
}

int cp_grad_flat_offsets(int n_tensors, const int64_t* lengths, int64_t* offsets) {
    if (!offsets) return fail(CP_ERR_INVALID, "grad_pack: null offsets");
    if (const char* e = cp_grad_layout(n_tensors, lengths, offsets, nullptr, nullptr)) return fail(CP_ERR_INVALID, e);
    return CP_OK;
}

size_t cp_grad_pack_table_bytes(int n_tensors, const int64_t* lengths, int* n_chunks) {
    long long nc = 0;
    const char* e = cp_grad_layout(n_tensors, lengths, nullptr, nullptr, &nc);
    if (!e && !n_chunks) e = "grad_pack: null n_chunks";
    if (e) {
        fail(CP_ERR_INVALID, e);
        return 0;
    }
    *n_chunks = (int)nc;  // at most 2^31 / CP_ADAM_CHUNK + n_tensors
    return cp_grad_pack_table_size(n_tensors, nc);
}

int cp_grad_pack_table_build(void* table, size_t table_bytes, int n_tensors, const void* const* src, const int64_t* lengths,
                             const int64_t* offsets, int* n_chunks) {
    if (!table || !src || !lengths || !offsets || !n_chunks) return fail(CP_ERR_INVALID, "grad_pack_table_build: null argument");
    long long nc = 0;
    if (const char* e = cp_grad_layout(n_tensors, lengths, nullptr, nullptr, &nc)) return fail(CP_ERR_INVALID, e);
    if (table_bytes < cp_grad_pack_table_size(n_tensors, nc)) return fail(CP_ERR_INVALID, "grad_pack_table_build: table buffer too small");
    if ((uintptr_t)table & 7) return fail(CP_ERR_INVALID, "grad_pack_table_build: table must be 8-byte aligned");
    if (const char* e = cp_grad_pack_table_fill(table, n_tensors, src, lengths, offsets)) return fail(CP_ERR_INVALID, e);
    *n_chunks = (int)nc;
    return CP_OK;
}

int cp_grad_pack(cp_stream_t stream, const void* table, int n_tensors, int n_chunks, float* flat, int64_t flat_elems, float scale) {
    if (!table || !flat) return fail(CP_ERR_INVALID, "grad_pack: null argument");
    if (n_tensors < 1) return fail(CP_ERR_INVALID, "grad_pack: n_tensors must be >= 1");
    if (n_chunks < 0) return fail(CP_ERR_INVALID, "grad_pack: n_chunks must be >= 0");
    if ((uintptr_t)table & 7) return fail(CP_ERR_INVALID, "grad_pack: table must be 8-byte aligned");
    if ((uintptr_t)flat & 15) return fail(CP_ERR_INVALID, "grad_pack: flat must be 16-byte aligned");
    if (!std::isfinite(scale)) return fail(CP_ERR_INVALID, "grad_pack: non-finite scale");
    if (flat_elems < cp_grad_min_flat_elems(n_tensors, n_chunks))
        return fail(CP_ERR_INVALID, "grad_pack: flat_elems is below every layout of n_tensors tensors and n_chunks chunks");
    const int rc = cp_launch_grad_pack((hipStream_t)stream, table, n_tensors, n_chunks, flat, (long long)flat_elems, scale);
    return rc == CP_OK ? CP_OK : fail(rc, "grad_pack: kernel launch failed");
}

}  // extern "C"
