// What the stand-alone operators share (ops.hip and the training operators dcn_bwd.hip, heads_bwd.hip, conv_bwd.hip,
// conv_bwd_lowc.hip, deconv_bwd.hip, batchnorm.hip, groupnorm.hip, gru_train.hip, pool.hip, stem_bwd.hip, optim.hip, grad_pack.hip): the launch check, the two
// fixed-order slab sums and the ConvParams of a convolution that runs as part of a gradient.  The summation orders are contract
// (the tests compare bitwise), so they are written here once.  The workspace carver, Carve, is in cp_common.h, where the target
// builders (pose_targets*.hip, train_inputs.hip) reach it without the engine's model header.
#pragma once
#include "engine_model.h"

inline bool launch_ok() { return hipGetLastError() == hipSuccess; }

// The two-level slab sum: a workgroup of 256 threads is 32 elements x 8 slab lanes (element threadIdx.x & 31, lane sl =
// threadIdx.x >> 5).  A lane folds acc = step(acc, s) over its slabs s = sl, sl + 8, ... in ascending order, starting from
// `init` (a serial walk over hundreds of slabs is one long chain of dependent adds behind strided loads); after one barrier the
// result is lane 0's value plus the lanes 1..7 in lane order.  Every thread of the workgroup must call it; every thread gets
// the result (the callers store it from the sl == 0 thread).  `valid`: the element exists; where not, no slab is read.  The
// caller puts a barrier before the next use of `red`.  T is float, or a small struct with operator+ that carries several
// sums through one walk over the slabs (batchnorm.hip's Sum2: one workgroup may own all of up to 2048 slabs, so a second
// walk would double that kernel's time).
template <class T, class F>
__device__ __forceinline__ T two_level_sum(T (&red)[256], bool valid, int nslab, T init, F step) {
    const int el = threadIdx.x & 31, sl = threadIdx.x >> 5;
    T acc = init;
    if (valid)
        for (int s = sl; s < nslab; s += 8) acc = step(acc, s);
    red[threadIdx.x] = acc;
    __syncthreads();
    T t = red[el];
    for (int j = 1; j < 8; ++j) t = t + red[j * 32 + el];
    return t;
}

// The serial slab sum: init + part[0][e] + part[1][e] + ..., slabs ascending, `stride` elements apart
__device__ __forceinline__ float serial_sum(const float* __restrict__ part, int nslab, size_t stride, size_t e, float init) {
    float v = init;
    for (int s = 0; s < nslab; ++s) v += part[(size_t)s * stride + e];
    return v;
}

// ConvParams of an exact-f32 convolution that runs as part of a gradient: src [B,H,W,Cin] NHWC with the float32 weight wp as
// cp_launch_pack_weight lays it out (conv_w_f32), out [B,Ho,Wo,Cout] NHWC.  dbg = 0: cp_set_debug's switches choose among
// inference kernels for A/B runs, and a gradient does not depend on them.
inline ConvParams grad_conv_params(int B, int H, int W, const float* src, int Cin, float* wp, const float* shift, int Cout, int KH,
                                   int KW, int stride, int pad, float* out) {
    ConvParams p = cp_engine::conv_params(B, H, W, &src, &Cin, 1, cp_engine::conv_w_f32(wp, nullptr, shift, Cin, Cout, KH, KW), stride,
                                          pad, CP_ACT_NONE);
    p.dbg = 0;
    p.out = out;
    p.store = CP_STORE_NHWC;
    p.ldo = Cout;
    return p;
}

// Regions of a [Cout,Cin,kh,kw] weight packed for the f16x3 kernels: two binary16 copies [cpad][kpad], the per-channel weight
// scales (2^e, 2^-e, scale * 2^-e), the input's |max| slot block, the fragment-ordered copies of the binary16 weights
constexpr size_t cp_amax_slot_bytes = (size_t)CP_AMAX_SUB * CP_AMAX_STRIDE * sizeof(unsigned);  // one |max| slot block
struct Pack16 {
    void *hi, *lo;
    float *wfwd, *winv, *sc16;
    unsigned* slot;
    void *fhi, *flo;
};
inline Pack16 carve_pack16(Carve& c, size_t kpad, size_t cpad) {
    Pack16 r;
    r.hi = c.take<void>(kpad * cpad * 2);
    r.lo = c.take<void>(kpad * cpad * 2);
    r.wfwd = c.take<float>(cpad * sizeof(float));
    r.winv = c.take<float>(cpad * sizeof(float));
    r.sc16 = c.take<float>(cpad * sizeof(float));
    r.slot = c.take<unsigned>(cp_amax_slot_bytes);
    r.fhi = c.take<void>(kpad * cpad * 2);
    r.flo = c.take<void>(kpad * cpad * 2);
    return r;
}
// ops.hip: the f16x3 operands of a forward convolution from its PyTorch-layout weight (what cp_conv2d_nhwc, cp_dcnv2_forward and
// cp_pose_heads_forward launch on)
int cp_pack_f16x3(const Pack16& r, const float* wt, const float* scale, int taps, cp_engine::ConvW& w, const float* x, size_t nx,
                  const float* om, size_t px, hipStream_t s);
