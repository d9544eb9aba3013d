// centerpose_amd — shared declarations for the HIP kernels (gfx950 / CDNA4 only).
//
// Activations are float32 NHWC ("pixel-major": all channels of one output pixel are
// contiguous).  That is the MI355X-first layout choice for this path: the DCNv2 bilinear gather
// and the implicit-GEMM loaders then read whole channel vectors (16 B per lane, 64-256 B per
// pixel) instead of the reference's per-channel NCHW planes (dcn_v2_im2col_cuda.cu:125-195
// touches 4 scattered floats per (channel, tap)).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/centerpose_hip_testing.h"  // CP_SEL_* (ConvParams::dbg)
#include "conv_variants.h"  // CP_VARIANT_*: the kernel variants the launchers below choose from

// The kernels of this library rely on the raw-buffer range check of the gfx9 / CDNA family as gfx950 implements it: a lane whose
// (voffset + soffset [+ immediate]) lies beyond the descriptor's num_records reads 0 -- per dword for a 16-byte access that
// straddles the end -- and its stores / LDS-DMA writes are dropped (zeros land in LDS).  Out-of-picture halo pixels, padded
// weight / bias rows, missing split-K slices (igemm.hip: splitk_epilogue4_kernel) and "invalid corner" gathers are all
// expressed that way (OOB / OOB_BASE in igemm16_common.h) instead of as branches.  Other architectures check differently
// (gfx10+ exclude soffset in some modes): refuse to build device code for anything else.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "centerpose_amd device code is written for gfx950 only (raw-buffer range-check semantics, MFMA shapes, LDS-DMA)"
#endif

#define CP_OK 0
#define CP_ERR_INVALID (-1)
#define CP_ERR_LAUNCH (-2)
#define CP_ERR_ALLOC (-3)
#define CP_ERR_STATE (-4)

enum CpAct : int {
    CP_ACT_NONE = 0,
    CP_ACT_RELU = 1,
    CP_ACT_SIGMOID = 2,       // all channels
    CP_ACT_SIGMOID_FROM = 3,  // sigmoid on channels >= act_from (DCN mask logits), identity below
};

enum CpStore : int {
    CP_STORE_NHWC = 0,  // out[(pixel) * ldo + coff + c]
    CP_STORE_NCHW = 1,  // out[((b * Cout_total) + coff + c) * HoWo + p]   (reference head layout)
};

#define CP_MAX_SRC 4
#define CP_MAX_HEAD_GROUP 12

// Bump carver over an operator's workspace.  Each operator describes its regions once, in a *_carve function: run on the
// caller's pointer it hands out the regions, run on nullptr it only counts, and *_workspace_bytes is `off` of that run -- the
// size and the carve-up cannot drift apart.  `end` is the unrounded end of the last region taken: the size of a workspace
// whose ABI does not round its last region.
struct Carve {
    char* base;
    size_t off = 0, end = 0;
    template <class T>
    T* take(size_t bytes) {
        T* p = base ? (T*)(base + off) : nullptr;
        end = off + bytes;
        off += (bytes + 255) / 256 * 256;
        return p;
    }
};

#ifdef __HIPCC__
// ---- ReLU and its gradient gate as the training operators compute them: torch's rules, under which a NaN stays a NaN ----
// relu(v) = 0 where v <= 0, else v: equal to fmaxf(v, 0.f) bit for bit on every number (-0 gives +0 either way), but a NaN
// passes -- fmaxf(NaN, 0) is 0, which would turn a poisoned activation into a healthy-looking dead one ("Non-finite
// values").  cp_relu_gate: threshold_backward, the gradient passes unless y <= 0, so it passes where y is NaN.
__device__ __forceinline__ float cp_relu(float v) { return v <= 0.f ? 0.f : v; }
__device__ __forceinline__ float cp_relu_gate(float g, float y) { return y <= 0.f ? 0.f : g; }
// ---- |max| tracking and power-of-two operand scaling for the split-f16 kernels (see ConvParams::in_amax) ----
// amax bits -> (2^e, 2^-e) with amax * 2^e in [2^14, 2^15): e = 14 - floor(log2(amax)).  Exponents are clamped so that
// both factors stay normal float32 numbers (amax = 0 or < 2^-111: 2^125; inf / NaN inputs stay inf / NaN).  The upper clamp
// leaves the largest binade [2^127, 2^128) at [2^15, 2^16) instead of [2^14, 2^15): still finite in binary16 -- the split's hi
// half is rounded toward zero, so it stops at 65504 and the residual (< 32) goes to the lo half.  An infinite amax gets the
// same factor 2^-112.  A limit of the mode: the forward kernels and the stride-1 data gradient form scale * inv
// (weight factor times this inverse) before they multiply the accumulator, which under- or overflows for operands near 2^-112
// against weights near 2^112 although the result would be an ordinary number; cp_scale_pow2 below is the form without it.
__device__ __forceinline__ void cp_amax_to_scale(unsigned amax_bits, float* fwd, float* inv) {
    int e = (int)((amax_bits >> 23) & 0xffu);
    e = e < 16 ? 16 : (e > 253 ? 253 : e);
    *fwd = __uint_as_float((unsigned)(268 - e) << 23);
    *inv = __uint_as_float((unsigned)(e - 14) << 23);
}
// v * a * b for two of the power-of-two factors above, as ONE exact scaling: the exponents are added as integers and applied by
// ldexpf.  Written v * a * b, the first product overflows where one operand is huge and the other tiny (grad_out near 2^127 with
// weights near 2^-100: acc * 2^112 is infinite although acc * 2^112 * 2^-115 is an ordinary number); a * b first has the mirror
// problem.  Equal to v * a * b bit for bit wherever no intermediate leaves the normal range.
__device__ __forceinline__ float cp_scale_pow2(float v, float a, float b) {
    return ldexpf(v, (int)((__float_as_uint(a) >> 23) & 0xffu) + (int)((__float_as_uint(b) >> 23) & 0xffu) - 254);
}
// A tensor's |max| lives in CP_AMAX_SUB sub-slots CP_AMAX_STRIDE uints apart (different cache lines): all waves of a
// small kernel finish at about the same time, all find the slot still at its old value and all issue their atomic --
// thousands of same-address atomics serialise at the memory side (measured: +10 us per kernel at batch 1).  Spreading
// the writers over 32 addresses by workgroup (one atomic per workgroup) cuts that to a handful per address; readers
// take the max.
#define CP_AMAX_SUB 32
#define CP_AMAX_STRIDE 2048  // = |max| slots (tensors) per forward pass
__device__ __forceinline__ unsigned cp_amax_read(const unsigned* slot) {
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < CP_AMAX_SUB; ++k) m = max(m, slot[k * CP_AMAX_STRIDE]);
    return m;
}
// Block-reduce the lanes' local max|v| (wave shuffle, then one LDS word per wave) and fold it into the block's sub-slot
// (float bits of non-negative numbers order like unsigned integers).  The sub-slot is read first: later blocks usually
// find their maximum covered and skip the atomic.  Every thread of the block must call it (it contains a barrier).
__device__ __forceinline__ void cp_amax_commit(unsigned* slot, float local) {
    __shared__ float cp_amax_red[16];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local = fmaxf(local, __shfl_xor(local, o, 64));
    if ((threadIdx.x & 63) == 0) cp_amax_red[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (int)(blockDim.x + 63) >> 6;
        float m = cp_amax_red[0];
        for (int i = 1; i < nw; ++i) m = fmaxf(m, cp_amax_red[i]);
        unsigned* sub = slot + (blockIdx.x & (CP_AMAX_SUB - 1)) * CP_AMAX_STRIDE;
        const unsigned b = __float_as_uint(m);
        if (b > __hip_atomic_load(sub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(sub, b);
    }
}

// Gate non-linearities of the fused ConvGRU epilogues (f16x3 mode): hardware exp2 / rcp, absolute error < 3e-7 (sigmoid)
// and < 6e-7 (tanh) against expf / tanhf, i.e. at float32 round-off of the gate values.  The library forms cost ~80 VALU
// instructions per output (range reduction, IEEE division, tanhf's branches) -- with 48 outputs per lane that was more
// vector-ALU time than the K loop has matrix time.  The exact-f32 mode and the stand-alone gate kernel keep expf / tanhf.
__device__ __forceinline__ float cp_fast_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}
__device__ __forceinline__ float cp_fast_tanh(float x) {
    return 2.f * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-2.8853900817779268f * x)) - 1.f;
}
#endif

// One implicit-GEMM convolution:  out[m, n] = act( (sum_k A[m,k] * Wp[k,n]) * scale[n] + shift[n] + res[m,n] )
//   m = output pixel (b, ho, wo);  k = (tap, ci) with ci fastest;  n = output channel.
// A is read on the fly from up to CP_MAX_SRC NHWC sources that form a virtual channel concat
// (Root's torch.cat, pose_dla_dcn.py:162), or — in DCN mode — produced by the modulated bilinear
// gather of the reference's deformable im2col (dcn_v2_im2col_cuda.cu:125-195) without ever
// materialising the `columns` buffer.
struct ConvParams {
    const float* src[CP_MAX_SRC];
    int src_c[CP_MAX_SRC];  // channels per source (multiples of 4)
    int nsrc;
    int Cin;  // total input channels
    int B, H, W, Ho, Wo;
    int KH, KW, stride, pad;
    int K;     // KH*KW*Cin (un-padded)
    int Kpad;  // rows of wp (multiple of BK)
    const float* wp;  // packed weights [Kpad][CoutPad]
    int Cout, CoutPad;
    const float* scale;  // [CoutPad] or nullptr (=1)
    const float* shift;  // [CoutPad] or nullptr (=0)
    const float* res;    // NHWC [M][res_ld] or nullptr
    int res_ld;
    int act;
    int act_from;
    float* out;
    int store;       // CpStore
    int ldo;         // NHWC: channel stride of out; NCHW: total channels of out tensor
    int coff;        // channel offset inside out
    const void* w16_hi;    // split-f16 path: packed weights [CoutPad][Kpad16] binary16 (hi / lo), or nullptr
    const void* w16_lo;
    // the same two arrays in MFMA B-operand order (cp_launch_frag16_repack), optional: dcn16p.hip loads its weight
    // fragments straight from them
    const void* w16f_hi;
    const void* w16f_lo;
    int Kpad16;
    // GroupNorm fusion (dlav1 heads, GN.py:4-9): the producing conv accumulates per-(image, group) sum / sum of
    // squares of its biased output into gn_stats[B][groups][2] (doubles, zeroed by the caller); the consuming 1x1
    // conv normalises + affine + ReLU on load from gn_in_mr[B][groups] = (mean, rstd).
    double* gn_stats;
    int gn_groups, gn_cpg;
    const float* gn_in_mr;
    const float* gn_in_gamma;
    const float* gn_in_beta;
    // the same fusion for the f16x3 1x1 kernel: the normalisation pre-folded per (image, channel) to y = relu(a*x + d),
    // planes [B][Cin] each (cp_launch_gn_affine)
    const float* gn_in_a;
    const float* gn_in_d;
    // fused ConvGRU step (convGRU.py:32-39) on the hidden-side 3x3 convolution: weights packed so that an N tile of 96
    // holds [r | z | n] of the same 32 channels; the epilogue reads gru_x3 ([M,192] = input-side pre-activations) and
    // gru_hprev ([M,64]) and writes h' = (1-z)*n + z*h into out ([M,64]).  The [M,192] hidden-side tensor never exists.
    const float* gru_x3;
    const float* gru_hprev;
    // deterministic split-K (few output tiles, long K: low-resolution layers at small batch): blockIdx.y = K slice,
    // raw accumulators go to partial[slice][M][CoutPad]; cp_launch_splitk_epilogue sums the slices in order and
    // applies the usual epilogue.
    int splitk;
    float* partial;
    // tile of a split-K launch when it should be smaller than the default 128 x cp_conv_tile_n(Cout) (0 = default): the slab
    // volume is slices x M x Cout x 4 bytes, and smaller tiles reach the same workgroup count with fewer slices
    int tile_m, tile_n;
    // Fused prediction head (dlav1 heads: conv3x3 -> ReLU -> conv1x1, pose_dla_dcn.py head Sequential): the 3x3 tile
    // is multiplied by the 1x1 weights inside the kernel and only [slices = CoutPad/128][fuse_c2][M] partial sums of the
    // final maps are written (fuse_out); cp_launch_head_reduce adds the slices + bias (+ sigmoid) into NCHW.  The
    // 256-channel hidden tensor never exists in memory.  fuse_w2_*: 1x1 weights packed as MFMA fragments
    // (cp_launch_pack_head_w2).
    const void* fuse_w2_hi;
    const void* fuse_w2_lo;
    float* fuse_out;
    int fuse_c2;
    // Several fused heads that read the same input in ONE launch (halo16.hip, EPI = 1): the 3x3 weights, scale / shift, 1x1
    // fragments and w2_inv tables of the heads are concatenated along N (CoutPad = sum of the heads' hidden widths); N
    // tile tn belongs to head g = tn / fuse_gtiles, whose final maps have fuse_gc2[g] channels and whose slabs start at
    // plane fuse_gbase[g] of fuse_out ([plane][M]; head g owns fuse_gtiles * fuse_gc2[g] planes, slice-major).
    // fuse_ngroups == 0: one head, fuse_c2 channels, planes from 0 (the layout above).
    int fuse_ngroups, fuse_gtiles;
    int fuse_gc2[CP_MAX_HEAD_GROUP];
    int fuse_gbase[CP_MAX_HEAD_GROUP];
    // fuse_final (halo16 grouped launch, Cin == 64): a workgroup stages its patch once, walks all fuse_gtiles hidden tiles of
    // its head and writes the finished maps -- sum of the tiles in index order + bias (+ sigmoid), NCHW, the arithmetic of
    // head_reduce_grouped_kernel -- so neither the slabs nor the reduction launch exist.  fuse_out is then unused.
    int fuse_final;
    int fuse_gsig[CP_MAX_HEAD_GROUP];
    const float* fuse_gbias[CP_MAX_HEAD_GROUP];
    float* fuse_gout[CP_MAX_HEAD_GROUP];
    // ---- range-safe split-f16 arithmetic (f16x3 kernels) ----
    // Binary16 only has 5 exponent bits, so the hi/lo split is exact to 2^-21 only while the operand sits well inside
    // the normal range.  Both operands are therefore pre-scaled by exact powers of two: weights per output channel at
    // pack time (the inverse is folded into `scale`, which for f16x3 launches points at scale * 2^-e_w), activations per
    // tensor at run time from the tensor's running |max| (in_amax: float bits of max|x| written by the producing
    // kernel's epilogue into a 4-byte slot; several sources of a virtual concat share the largest).  The loader
    // multiplies by 2^e_a before the split and the epilogue by 2^-e_a: every partial sum is scaled by the same power
    // of two, so results are bit-identical to the unscaled arithmetic wherever that one was inside the normal range.
    const unsigned* in_amax[CP_MAX_SRC];  // nullptr: operand used as is (scale 1)
    unsigned* out_amax;                   // nullptr: the output's |max| is not tracked
    const float* fuse_w2_inv;             // fused head: 2^-e of the 1x1 weights per final channel [32]
    int dbg;  // kernel-selection switches of cp_set_debug (CP_SEL_*, include/centerpose_hip_testing.h)
    const float* offmask;  // DCN mode: NHWC [B,H,W,32] = 18 offsets (dh,dw interleaved per tap) + 9 masks (already sigmoided) + 5 pad
    // Fused head over a LIST of output pixels instead of the whole map (igemm16.hip, cp_launch_conv16_fused_head_rows): GEMM row m
    // is image b = m / rows_per_image, pixel row_index[b * row_index_stride + m % rows_per_image] (= ho * Wo + wo, clamped into
    // the map), M = B * rows_per_image.  Taps outside the image are zero as everywhere; a pixel listed twice is computed twice.
    // Slabs as above with this M; with fuse_ngroups > 0 the grouped plane layout (fuse_gtiles / fuse_gc2 / fuse_gbase) and
    // fuse_w2_inv[g * 64 + c].
    const int* row_index;
    int rows_per_image, row_index_stride;
    // IDAUp's up-sample + add in the epilogue of the DCN that produces `add` (dcn16t.hip, cp_dcn16t_upadd_supported): the kernel
    // writes u = act(...) + up(up_t) (upadd_common.h) to `out` and |max| of u to out_amax; its own output is never stored.
    // up_t: NHWC [B, H / up_f, W / up_f, up_ld] with Cout valid channels, complete in memory before the launch; up_wt: the
    // depth-wise kernels as [tap = ky * 2 up_f + kx][Cout].  up_t == nullptr: a plain launch.
    const float* up_t;
    const float* up_wt;
    int up_ld, up_f;
    // The 1x1 projection of a DLA level entry (Tree.project: conv1x1 + BatchNorm, no activation) computed by the 3x3 launch that
    // would otherwise read it back as `res` (halo16.hip, cp_halo16_project_supported): after its own K loop the workgroup runs the
    // pj_c-deep product of its 8 x 16 pixels of pj_src into a second accumulator set -- pw16.hip's operands, K order and term
    // order, so the value is the one the stand-alone launch stores -- and the epilogue adds acc2 * pj_scale * 2^-e + pj_shift
    // where it adds `res`.  The projected tensor never exists.  pj_src: NHWC [B, H, W, pj_c] at output resolution, pj_c a
    // multiple of 32; pj_amax: its |max| slot (nullptr: used as is); pj_w_*: the projection's weights in fragment order
    // (cp_launch_frag16_repack), CoutPad rows of pj_c; pj_scale (already times 2^-e_w) / pj_shift: [CoutPad] or nullptr.
    // pj_src == nullptr: a plain launch.  `res` must be nullptr with it.
    const float* pj_src;
    int pj_c;
    const unsigned* pj_amax;
    const void* pj_w_hi;
    const void* pj_w_lo;
    const float* pj_scale;
    const float* pj_shift;
    // A second, 2x2 max-pooled copy of the output written by the launch that produces it (pw16.hip: pw16s_kernel's POOL
    // instances, cp_pw16_pool_supported): NHWC [B, Ho / 2, Wo / 2, ldo], each value the maximum of the four activated outputs of
    // its window -- what cp_launch_maxpool2 makes of `out`, without reading `out` back.  Its |max| is bounded by out_amax's.
    // pool_out == nullptr: a plain launch.
    float* pool_out;
};

int cp_launch_conv(const ConvParams& p, hipStream_t stream);
// Tile N-width the launcher will pick for `cout` (weights must be padded to a multiple of it); cp_conv16_tile_n: of the f16x3 launch
int cp_conv_tile_n(int cout);
int cp_conv16_tile_n(const ConvParams& p);
// The selectors: the CP_VARIANT_* (conv_variants.h) that cp_launch_conv / cp_launch_conv16 run p on -- the launchers dispatch on this answer
int cp_conv_variant(const ConvParams& p);
int cp_launch_splitk_epilogue(const ConvParams& p, hipStream_t stream);
// K steps (of 16 for the f32 kernels, 32 for f16x3) and output tiles of the launch cp_launch_conv[16] would make
void cp_conv_geometry(const ConvParams& p, bool f16x3, int* tiles, int* nk);
const char* cp_conv_variant_name(int v);
// split-f16 ("f16x3") implicit GEMM (igemm16.hip)
bool cp_conv16_supported(const ConvParams& p);
int cp_launch_conv16(const ConvParams& p, hipStream_t stream);
int cp_conv16_variant(const ConvParams& p);
bool cp_conv16_project_supported(const ConvParams& p);  // ConvParams::pj_src: the launch lands on a kernel that computes it
// halo-resident 3x3 / stride-1 convolution (halo16.hip): eligibility and launch (bn = N tile 32 / 64 / 128)
bool cp_halo16_supported(const ConvParams& p);
bool cp_halo16_fused_head_supported(const ConvParams& p);
int cp_launch_halo16_fused_head(const ConvParams& p, hipStream_t stream);
bool cp_halo16_gru_supported(const ConvParams& p);
int cp_launch_halo16_gru(const ConvParams& p, hipStream_t stream);
int cp_launch_halo16(const ConvParams& p, int bn, hipStream_t stream);
bool cp_halo16_project_supported(const ConvParams& p, int bn);  // ... with ConvParams::pj_src (the 64- and 128-wide N tiles)
// strm16.hip: 64 -> <= 32 channel 3x3 / stride-1 layers (DCN offset / mask convolutions) as wave-private row streams, weights in LDS
bool cp_strm16_supported(const ConvParams& p);
int cp_strm16_jobs(const ConvParams& p);
int cp_launch_strm16(const ConvParams& p, hipStream_t stream);
// fused DCNv2 gather + contraction (dcn16.hip); bn = N tile (64 / 128)
int cp_launch_dcn16(const ConvParams& p, int bn, hipStream_t stream);
// pw16.hip: 1x1 / stride-1 layers (incl. virtual concats) as a register-only stream, weight fragments from w16f_*
bool cp_pw16_supported(const ConvParams& p);
bool cp_pw16_pool_supported(const ConvParams& p);  // ... and can write ConvParams::pool_out (whole-line loads, Ho even, Wo % 16 == 0)
int cp_launch_pw16(const ConvParams& p, hipStream_t stream);
// dcn16p.hip: patch-resident DCNv2 (gather from an LDS-staged halo); N tile 64, or 128 (`wide`, NT = 4) where the selector, asking
// cp_dcn16p_wide, chose CP_VARIANT_DCN16PW
bool cp_dcn16p_supported(const ConvParams& p);
int cp_dcn16p_blocks(const ConvParams& p);
bool cp_dcn16p_wide(const ConvParams& p);
int cp_launch_dcn16p(const ConvParams& p, bool wide, hipStream_t stream);
// dcn16s.hip: the same gather as a persistent kernel with the halo streamed by LDS-DMA into two 16-channel buffers
// (launches with several (patch, N tile) items per resident workgroup)
bool cp_dcn16s_supported(const ConvParams& p);
int cp_dcn16s_items(const ConvParams& p);
int cp_launch_dcn16s(const ConvParams& p, hipStream_t stream);
int cp_launch_frag16_repack(const void* w16, void* w16f, int CoutPad, int Kpad16, hipStream_t s);
// dcn16t.hip: dcn16p's gather written for three workgroups per CU (16-channel chunks, one gather set, two weight sets)
bool cp_dcn16t_supported(const ConvParams& p);
bool cp_dcn16t_upadd_supported(const ConvParams& p);  // ... with ConvParams::up_t (one 64-channel N tile, up_f 2 or 4)
int cp_launch_dcn16t(const ConvParams& p, hipStream_t stream);
// `fwd` (may be nullptr = 1): per-output-channel power-of-two factor applied before the split, indexed [coff + co]
int cp_launch_pack_weight16(const float* w, void* hi, void* lo, int Cout, int Cin, int taps, int Kpad16, int coff,
                            const float* fwd, hipStream_t s);
// per-output-channel power-of-two scale of a [Cout][per] weight: fwd[co] = 2^e with max|w[co,:]| * 2^e in [2^14, 2^15),
// inv[co] = 2^-e (all-zero rows: 1)
int cp_launch_weight_scale(const float* w, int Cout, int per, float* fwd, float* inv, hipStream_t s);
// out[i] = (scale ? scale[i] : 1) * inv[i]
int cp_launch_scale16(const float* scale, const float* inv, float* out, int n, hipStream_t s);
// |max| of x[0..n) folded into the slot's sub-slots (CP_AMAX_SUB x CP_AMAX_STRIDE uints, zeroed by the caller);
// n % 4 == 0, 16-byte aligned
int cp_launch_absmax(const float* x, size_t n, unsigned* slot, hipStream_t s);
// fused head (see ConvParams::fuse_*): is this 3x3 (+ReLU) -> 1x1 pair eligible; launch; 1x1 weight packing
// (w1: [C2][Chid] float32 -> two arrays of Chid*32 binary16); slice reduction + bias (+ sigmoid) -> NCHW
bool cp_head_fuse_supported(const ConvParams& p, int c2);
int cp_launch_conv16_fused_head(const ConvParams& p, hipStream_t stream);
// the same head at the pixels of ConvParams::row_index only (always the per-tap implicit GEMM: scattered pixels share no patch)
int cp_launch_conv16_fused_head_rows(const ConvParams& p, hipStream_t stream);
// w2_inv: [32] floats, receives 2^-e per final channel (the packed rows are scaled by 2^e)
int cp_launch_pack_head_w2(const float* w1, void* hi, void* lo, float* w2_inv, int C2, int Chid, hipStream_t s);
int cp_launch_head_reduce(const float* slabs, const float* bias, float* out_nchw, int slices, int C2, int B, int HW,
                          int sigmoid, hipStream_t s);
// the same for a group of heads in one launch: head g reads planes base[g] .. base[g] + slices * c2[g] of `slabs`
struct HeadReduceGroup {
    int n, slices;
    int c2[CP_MAX_HEAD_GROUP], base[CP_MAX_HEAD_GROUP], sigmoid[CP_MAX_HEAD_GROUP];
    const float* bias[CP_MAX_HEAD_GROUP];
    float* out[CP_MAX_HEAD_GROUP];
};
int cp_launch_head_reduce_grouped(const float* slabs, const HeadReduceGroup& g, int B, int HW, hipStream_t s);
int cp_launch_conv16_gru(const ConvParams& p, hipStream_t stream);
int cp_conv16_fused_head_variant(const ConvParams& p);  // what cp_launch_conv16_fused_head / _gru run p on
int cp_conv16_gru_variant(const ConvParams& p);
// direct low-channel convolutions of the network's first three layers in f16x3 mode (lowc.hip).
// kind: 0 stem 7x7 (NCHW input, `planes` <= 4) -> 16; 1 level0 3x3 16->16; 2 level1 3x3 stride 2 16->32
size_t cp_lowc_weight_halfs(int kind);
// fwd: per-output-channel power-of-two weight pre-scale (cp_launch_weight_scale) or nullptr; `scale` of cp_launch_lowc
// must then carry the inverse.  in_amax / out_amax: see ConvParams.
int cp_launch_pack_lowc(int kind, const float* w, void* hi, void* lo, const float* fwd, int cin, hipStream_t s);
int cp_launch_lowc(int kind, const float* in, float* out, const void* w_hi, const void* w_lo, const float* scale,
                   const float* shift, const unsigned* in_amax, unsigned* out_amax, int B, int H, int W, int planes,
                   hipStream_t s, float* pool_out = nullptr);
// pool_out (kind 5 only, cp_lowc_pool_supported): NHWC [B][Ho / 2][Wo / 2][32] receives the 2x2 max-pooled copy of `out`, written
// by the same launch (what cp_launch_maxpool2 makes of `out`); its |max| is bounded by out_amax's
bool cp_lowc_pool_supported(int kind, int H, int W);
// stem + level0 in one launch (lowc.hip: lowc2_kernel): the 16-channel full-resolution tensor between them is never stored
int cp_launch_lowc_fused(const float* in, float* out, const void* w0_hi, const void* w0_lo, const float* scale0, const float* shift0,
                         const void* w1_hi, const void* w1_lo, const float* scale1, const float* shift1, float bound_l, float bound_s,
                         const unsigned* in_amax, unsigned* out_amax, int B, int H, int W, int planes, hipStream_t s);
// dense ConvTranspose2d(k=4, stride=2, pad=1) + per-channel affine (+ ReLU), four sub-pixel classes in one launch (deconv16.hip).
// Weights packed by cp_launch_pack_deconv from PyTorch [Cin][Cout][4][4]: wf float32 and / or hi / lo binary16, each
// [4][cp_deconv_cout_pad(Cout)][4*Cin]; inv[co] = 2^-e of the binary16 rows (f16x3 `scale` must carry it).  Cin % 32 == 0.
struct DeconvLaunch {
    const float* x;  // [B,H,W,Cin]
    const float* wf;
    const void* w_hi;
    const void* w_lo;
    const float* scale;  // [CoutPad] or nullptr
    const float* shift;  // [CoutPad] or nullptr
    float* out;          // [B,2H,2W,Cout]
    const unsigned* in_amax;  // f16x3: the input's |max| slot (nullptr: operand used as is)
    unsigned* out_amax;       // the output's |max| slot or nullptr
    int B, H, W, Cin, Cout, relu, f16x3;
};
int cp_deconv_cout_pad(int Cout);
int cp_launch_pack_deconv(const float* w, float* wf, void* hi, void* lo, float* inv, int Cin, int Cout, hipStream_t s);
int cp_launch_deconv(const DeconvLaunch& l, hipStream_t s);
#define CP_PREC_F32 0
#define CP_PREC_F16X3 1

// ---- element-wise / data-movement kernels (ewise.hip) ----
int cp_launch_nchw_to_nhwc(const float* in, float* out, int B, int C, int H, int W, int Cpad, hipStream_t s);
int cp_launch_nhwc_to_nchw(const float* in, float* out, int B, int C, int H, int W, int ldi, hipStream_t s);
int cp_launch_maxpool2(const float* in, float* out, int B, int H, int W, int C, hipStream_t s);
// MaxPool2d(3, stride 2, pad 1) (resnet_dcn.py PoseResNet.maxpool): padding is -inf; optional |max| slot of the output
int cp_launch_maxpool3s2(const float* in, float* out, int B, int H, int W, int C, unsigned* out_amax, hipStream_t s);
// the element-wise producers below take an optional |max| slot for their output (ConvParams::out_amax)
// depth-wise ConvTranspose2d(k=2f, stride=f, pad=f/2) of `in` [B,H,W,C] plus `add` [B,fH,fW,C] -> out
int cp_launch_upsample_add(const float* in, const float* w, const float* add, float* out, int B, int H, int W,
                           int C, int f, unsigned* out_amax, hipStream_t s);
int cp_launch_add_relu_sum(const float* a, const float* b, const float* c, const float* d, float* out, size_t n,
                           unsigned* out_amax, hipStream_t s);
// hourglass merge: out[B,2H,2W,C] = up1 + nearest-x2(low[B,H,W,C])  (large_hourglass.py:186-188)
int cp_launch_upsample2_nearest_add(const float* up1, const float* low, float* out, int B, int H, int W, int C,
                                    unsigned* out_amax, hipStream_t s);
// its gradient with respect to low: grad_low[B,H,W,C] = the four grad_out[B,2H,2W,C] elements of each 2x2 cell, in a fixed order
int cp_launch_upsample2_nearest_add_backward(const float* grad_out, float* grad_low, int B, int H, int W, int C, hipStream_t s);
// ConvGRU gates (convGRU.py:32-39).  x3/h3: [M,192] = (r,z,n) pre-activations, h: [M,64]
int cp_launch_gru_gate(const float* x3, const float* h3, const float* hprev, float* hout, size_t M, unsigned* out_amax,
                       hipStream_t s);
// GroupNorm(32 groups) over NHWC [B, HW, C]: stats then in-place normalise + affine + ReLU
int cp_launch_groupnorm_relu(float* x, const float* gamma, const float* beta, double* stats_ws, int B, int HW, int C,
                             int groups, float eps, unsigned* out_amax, hipStream_t s);
// (sum, sumsq) doubles -> (mean, rstd) floats per (image, group)
// (sum, sum of squares) per (image, group) -> per (image, channel) affine a = rstd*gamma, d = beta - mean*rstd*gamma
// x_amax / y_amax (optional): |max| slot of the un-normalised tensor, and the slot that receives the bound
// max over (image, channel) of |a| * max|x| + |d| >= max|relu(a*x + d)| for the consumer's activation pre-scale
int cp_launch_gn_final(const float* x, const float* ga, const float* gd, const float* wp, const float* bias, float* out,
                       int B, int HW, int C, int N, int wld, int sigmoid, hipStream_t s);
int cp_launch_gn_affine(const double* stats, const float* gamma, const float* beta, float* a, float* d, int B, int C,
                        int groups, double count, float eps, const unsigned* x_amax, unsigned* y_amax, hipStream_t s);
int cp_launch_gn_finalize(const double* stats, float* mr, int n, double count, float eps, hipStream_t s);
// PyTorch [Cout][Cin][taps] weights -> packed GEMM operand (buffer must be pre-zeroed for padding)
int cp_launch_pack_weight(const float* w, float* wp, int Cout, int Cin, int taps, int CinP, int CoutPad, int coff,
                          hipStream_t s);

// ---- decode (decode.hip) ----
// detection record: 118 float32 per detection, J = 8 joints (field order of decode.py:347-361)
#define CP_DET_BBOX 0
#define CP_DET_SCORE 4
#define CP_DET_KPS 5
#define CP_DET_CLS 21
#define CP_DET_SCALE 22
#define CP_DET_SCALE_UNC 25
#define CP_DET_TRACKING 28
#define CP_DET_TRACKING_HP 30
#define CP_DET_KPS_DISP_MEAN 46
#define CP_DET_KPS_DISP_STD 62
#define CP_DET_KPS_HM_MEAN 78
#define CP_DET_KPS_HM_STD 94
#define CP_DET_KPS_HM_HEIGHT 110
#define CP_DET_STRIDE 118
size_t cp_decode_ws_bytes(int B, int J, int K);
int cp_launch_decode(hipStream_t s, int B, int J, int H, int W, float* hm, const float* hps, const float* wh,
                     const float* hps_unc, const float* scale, const float* scale_unc, const float* reg, float* hm_hp,
                     const float* hp_offset, const float* tracking, const float* tracking_hp, int K, int rep_mode,
                     int fit_gaussian, float balance, int legacy_bool_mask, int apply_sigmoid, float* det, void* ws);
// The two halves of either decode.  Peaks: NMS + top-K of hm and the J hm_hp maps -> pk_score / pk_ind [B][J+1][K] (`cand`: the
// tiled form's candidate buffer = its workspace behind the peak tables; unused up to 32768 pixels).  Assoc: the records from
// the peak tables.  compact == 0: the regression heads are dense NCHW maps read at pk_ind; compact != 0: they are tables holding
// the values AT the peaks -- [B][C][K] (entry k = the head at pk_ind[b][0][k]) for the centre-indexed heads and
// hp_offset [B][J][2][K] (entry k of joint j = the head at pk_ind[b][j + 1][k]); hm_hp stays the dense map.
int cp_launch_decode_peaks(hipStream_t s, int B, int J, int H, int W, float* hm, float* hm_hp, int K, int apply_sigmoid,
                           float* pk_score, int* pk_ind, void* cand);
int cp_launch_decode_assoc(hipStream_t s, int B, int J, int H, int W, const float* hps, const float* wh, const float* hps_unc,
                           const float* scale, const float* scale_unc, const float* reg, const float* hm_hp,
                           const float* hp_offset, const float* tracking, const float* tracking_hp, const float* pk_score,
                           const int* pk_ind, int K, int rep_mode, int fit_gaussian, float balance, int legacy_bool_mask,
                           int compact, float* det);
size_t cp_decode_cand_bytes(int B, int J, int H, int W, int K);  // 0 up to 32768 pixels; (size_t)-1: unsupported shape
// tiled peaks (any W % 4 == 0, W <= 4096, K <= H*W <= 2^20; decode.hip): 0 bytes = unsupported shape
size_t cp_decode_tiled_ws_bytes(int B, int J, int H, int W, int K);
int cp_launch_decode_tiled(hipStream_t s, int B, int J, int H, int W, float* hm, const float* hps, const float* wh,
                           const float* hps_unc, const float* scale, const float* scale_unc, const float* reg, float* hm_hp,
                           const float* hp_offset, const float* tracking, const float* tracking_hp, int K, int rep_mode,
                           int fit_gaussian, float balance, int legacy_bool_mask, int apply_sigmoid, float* det, void* ws);

// ---- generic DCNv2 forward on the reference's NCHW layouts (dcn_generic.hip): any C / kernel / stride / dilation / dg ----
int cp_launch_dcn_generic(hipStream_t s, const float* x, const float* w, const float* bias, const float* offset,
                          const float* mask, float* out, int B, int C, int H, int W, int Co, int Ho, int Wo, int kh, int kw,
                          int sh, int sw, int ph, int pw, int dh, int dw, int dg);

// ---- DCNv2 backward (dcn_bwd.hip): every shape the forward accepts; NCHW in and out ----
struct DcnBwdArgs {
    const float *input, *weight, *offset, *mask, *grad_output;
    float *grad_input, *grad_offset, *grad_mask, *grad_weight, *grad_bias;
    int B, C, H, W, Co, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, dg;
};
bool cp_dcn_backward_fast(int C, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int dg);
// `precision` (CP_PREC_*): CP_PREC_F16X3 runs the two contractions of the fast geometry on the split-binary16 kernels of
// dcn_bwd16.hip and conv_bwd16.hip; the data side, grad_bias and the generic geometry are float32 in either mode.
// cp_dcn_backward_prec_mask: bit 0 = the weight gradient, bit 1 = grad_col runs in f16x3 (0 for CP_PREC_F32 and off the fast
// geometry; the chunk plan is the same on both paths, so the mask does not depend on `deterministic`).
size_t cp_dcn_backward_ws_bytes(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                                int dw, int dg, int precision);
int cp_launch_dcn_backward(hipStream_t s, const DcnBwdArgs& a, void* ws, int precision);
// the deterministic form (fast geometry only: the callers check cp_dcn_backward_fast first)
size_t cp_dcn_backward_det_ws_bytes(int B, int C, int H, int W, int Co, int precision);
int cp_launch_dcn_backward_det(hipStream_t s, const DcnBwdArgs& a, void* ws, int precision);
int cp_dcn_backward_prec_mask(int B, int C, int H, int W, int Co, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                              int dg, int precision);
// dcn_bwd16.hip: the pieces of the f16x3 mode on the fast geometry.  Slots are |max| slots of one zeroed block.
//   go_pad    go_t [B HW][CoP] = grad_output [B,Co,HW] transposed, zeros in the pad lanes (CoP % 32 == 0), and its |max|
//   col16     the modulated deformable im2col of images b0 .. b0 + nb - 1 as split dwords [image][pixel][tap][C], times 2^e of the
//             bound |max x| * |max mask| (x_amax, m_amax)
//   wgrad16   slab[s][co][k] (+)= sum over the pixels of slab s of go16[q][co] * col16[q][k], q < Q pixels from the pointers
//   reduce    grad_weight[co][c][tap] = (the slabs' two-level sum) * 2^-e_g * 2^-e_col
struct DcnWgrad16Plan {
    int slab_px, nslab, nh, jobs;
};
DcnWgrad16Plan cp_dcn_wgrad16_plan(size_t Q, int C, int CoP);  // Q: the pixels of a full chunk
int cp_launch_dcn_go_pad(hipStream_t s, const float* go, float* go_t, int B, int Co, int CoP, int HW, unsigned* slot);
int cp_launch_dcn_col16(hipStream_t s, const float* xh, const float* off, const float* mask, uint32_t* col16, const unsigned* x_amax,
                        const unsigned* m_amax, int b0, int nb, int C, int H, int W);
int cp_launch_dcn_wgrad16_slabs(hipStream_t s, const uint32_t* go16, const uint32_t* col16, float* slab, int Q, int C, int CoP,
                                const DcnWgrad16Plan& P, int accum);
int cp_launch_dcn_wgrad16_reduce(hipStream_t s, const float* slab, float* gw, int nslab, int Co, int CoP, int C,
                                 const unsigned* g_amax, const unsigned* x_amax, const unsigned* m_amax);

// ---- prediction-head block backward (heads_bwd.hip): n heads conv3x3 -> ReLU -> conv1x1 on one NHWC feature map ----
struct PoseHeadsArgs {
    const float* feat;          // [B,H,W,Cin]
    int n;                      // heads
    const float* const* w0;     // [hid,Cin,3,3] per head (PyTorch layout)
    const float* const* b0;     // [hid]
    const float* const* w1;     // [classes_i,hid]
    const float* const* b1;     // [classes_i]
    const int* classes;
    int B, H, W, Cin, hid;
};
int cp_pose_heads_chunk(int B, int H, int W, int hid);  // images whose hidden layer is materialised at a time
// `precision` (CP_PREC_*): CP_PREC_F16X3 runs the three wide contractions of a head -- the recomputed hidden layer, the 3x3
// weight gradient and the data gradient -- on the split-binary16 kernels (igemm16.hip's, conv_bwd16.hip's); the gate, grad_w1
// and the bias gradients are float32 in either mode.  cp_pose_heads_backward_mask: bit 0 = the weight gradient, bit 1 = the data
// gradient, bit 2 = the hidden layer runs in f16x3 (0 for CP_PREC_F32).
size_t cp_pose_heads_backward_ws_bytes(int B, int H, int W, int Cin, int hid, int max_classes, int precision);
int cp_pose_heads_backward_mask(int B, int H, int W, int Cin, int hid, int precision);
// grad_out[i] NCHW or nullptr (zero parameter gradients, no contribution); grad_feat NHWC or nullptr (not computed)
int cp_launch_pose_heads_backward(hipStream_t s, const PoseHeadsArgs& a, const float* const* grad_out, float* const* grad_w0,
                                  float* const* grad_b0, float* const* grad_w1, float* const* grad_b1, float* grad_feat,
                                  void* ws, int precision);

// ---- Conv2d backward (conv_bwd.hip): gradients of out = conv2d(x, w) + bias on the forward's NHWC layouts, float32 ----
struct ConvBwdArgs {
    const float *x, *w, *y, *go;  // y (the activated forward output) or nullptr: grad_out is gated by y > 0
    float *gx, *gw, *gb;          // gx / gb nullptr: not computed
    int B, H, W, Cin, Cout, KH, KW, stride, pad;
};
bool cp_conv_backward_mfma(int Cin, int KH, int KW, int stride, int pad);  // the geometry takes the MFMA kernels
// the geometry takes conv_bwd_lowc.hip's kernels: 3x3 / pad 1, stride 1 or 2, 16 -> 16 or 32, at least 4096 output pixels
bool cp_conv_backward_lowc(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
// CP_CONV_BWD_*: the path cp_launch_conv_backward takes (what cp_conv2d_backward_path reports); a valid geometry is assumed
int cp_conv_backward_path(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad);
// `precision` (CP_PREC_*): CP_PREC_F16X3 runs the MFMA path's two contractions on the split-binary16 kernels of conv_bwd16.hip;
// the other paths, the gate, the pad lanes and grad_bias are float32 in either mode.  cp_conv_backward_prec_mask: bit 0 = the
// weight gradient, bit 1 = the data gradient runs in f16x3 (0 for CP_PREC_F32 and off the MFMA path).
size_t cp_conv_backward_ws_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int need_grad_x,
                                 int precision);
int cp_launch_conv_backward(hipStream_t s, const ConvBwdArgs& a, void* ws, int precision);
int cp_conv_backward_prec_mask(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int precision);
// Its two MFMA contractions (cp_conv_backward_mfma geometries) as building blocks: cp_launch_conv_backward is made of them, and
// heads_bwd.hip runs them per head and chunk of images.  They read the geometry, x, gw and gx of `a` and, in place of a.go,
// gs [B,Ho,Wo,CoP]: grad_out already gated, CoP = Cout rounded up to 32 with zeros in the pad lanes.
struct ConvWgradPlan {
    int rows_per_slab, slabs, jobs;  // output rows per slab, slabs, wave jobs of wgrad_kernel
    size_t slab_bytes;               // the slab buffer (an upper bound of slabs x CoP x taps Cin x 4, monotone in rows)
};
ConvWgradPlan cp_conv_wgrad_plan(size_t rows, int Cin, int CoP, int taps);  // rows = B x Ho
// a.gw = (accum ? a.gw : 0) + the slabs' sum.  P may have been planned for more rows than a.B x Ho (a partial last chunk).
// `h` (f16x3): the split operands of conv_bwd16.hip in place of gs and a.x -- one dword per element, binary16 hi | lo << 16 of
// the element times 2^e from the tensor's |max| slot (cp_launch_absmax32, then cp_launch_split16); the slabs' sum is multiplied
// by 2^-(e_g + e_x) before it is stored or accumulated.  nullptr: float32.
struct ConvWgrad16 {
    const uint32_t *gs16, *x16;        // [B,Ho,Wo,CoP], [B,H,W,Cin]; x16 nullptr: a.x is scaled and split inside the kernel
    const unsigned *gs_amax, *x_amax;  // their |max| slots (CP_AMAX_SUB sub-slots each)
};
int cp_launch_conv_wgrad(hipStream_t s, const ConvBwdArgs& a, const float* gs, int CoP, const ConvWgradPlan& P, float* slab,
                         int accum, const ConvWgrad16* h = nullptr);
// Stride 1: w in the data gradient's operand form wB (any contents before), once per weight; then a.gx = gs (*) w^T (+ res
// [B,H,W,Cin], which may be a.gx itself) per launch.  precision CP_PREC_F16X3 packs the split-binary16 operand of igemm16.hip
// instead (a power-of-two scale per input channel of the layer); the launch then takes gs's |max| slot, and is only valid where
// cp_conv_dgrad16_s1_supported says so.
size_t cp_conv_dgrad_pack_bytes(int Cin, int CoP, int taps, int precision);
int cp_launch_conv_dgrad_pack(hipStream_t s, const float* w, float* wB, int Cin, int Cout, int CoP, int taps, int precision);
int cp_launch_conv_dgrad_s1(hipStream_t s, const ConvBwdArgs& a, const float* gs, int CoP, const float* wB, const float* res,
                            const unsigned* gs_amax = nullptr);  // gs_amax given: wB is the f16x3 pack
// conv_bwd16.hip: the pieces of the f16x3 mode.  |max| of x[0..n) into a zeroed slot; dst[i] = split(src[i] * 2^e of the slot);
// the slab kernel of the weight gradient; the data gradient's packed weight (stride 1 or 2), the stride-1 launch's eligibility
// (host arithmetic: cp_conv16_supported on the launch it would make) and the two launches.
int cp_launch_absmax32(const float* x, size_t n, unsigned* slot, hipStream_t s);
int cp_launch_split16(const float* src, uint32_t* dst, size_t n, const unsigned* slot, hipStream_t s);
int cp_launch_conv_wgrad16_slabs(hipStream_t s, const ConvBwdArgs& a, const ConvWgrad16& h, int CoP, const ConvWgradPlan& P, float* slab);
size_t cp_conv_dgrad16_pack_bytes(int Cin, int CoP, int taps, int stride);
int cp_launch_conv_dgrad16_pack(hipStream_t s, const float* w, void* wB, int Cin, int Cout, int CoP, int taps, int stride);
bool cp_conv_dgrad16_s1_supported(int B, int H, int W, int Cin, int CoP, int K);
int cp_launch_conv_dgrad16_s1(hipStream_t s, const ConvBwdArgs& a, const float* gs, int CoP, const void* wB, const float* res,
                              const unsigned* gs_amax);
int cp_launch_conv_dgrad16_s2(hipStream_t s, const ConvBwdArgs& a, const uint32_t* gs16, int CoP, const void* wB, const unsigned* gs_amax);
// The low-channel 3x3 path (conv_bwd_lowc.hip; cp_conv_backward_lowc geometries, CoP == Cout).  A workgroup walks a contiguous
// run of `tiles_per_wg` tiles; the weight gradient's workgroups are its slabs [Cout][9 x 16], which the caller sums
// (wgrad_reduce_kernel's layout and order).
struct ConvLowcPlan {
    int tiles_y, tiles_x, tiles, tiles_per_wg, wgs;
};
ConvLowcPlan cp_conv_lowc_wgrad_plan(int B, int Ho, int Wo, int stride);
ConvLowcPlan cp_conv_lowc_dgrad_plan(int B, int H, int W, int stride);
size_t cp_conv_lowc_slab_bytes(int B, int Ho, int Wo, int Cout, int stride);  // an upper bound of wgs slabs, monotone in B
int cp_launch_conv_lowc_wgrad(hipStream_t s, const ConvBwdArgs& a, const float* gs, const ConvLowcPlan& P, float* slab);
int cp_launch_conv_lowc_dgrad(hipStream_t s, const ConvBwdArgs& a, const float* gs);
// out[c] = sum over images and pixels of g [B,C,HW] (NCHW): a bias gradient, in a fixed order (dcn_bwd.hip, heads_bwd.hip)
int cp_launch_rowsum_nchw(const float* g, float* out, int B, int C, int HW, hipStream_t s);

// ---- ConvTranspose2d backward (deconv_bwd.hip): IDAUp's depth-wise `up` (k = 2 stride, pad = stride / 2, groups = C) and the
// dense k 4 / stride 2 / pad 1 layer, on the forward's NHWC layouts, float32 or (dense) f16x3 ----
#define CP_DECONV_DW_TABLE_BYTES 61440  // the depth-wise kernels stage w as [k k][C] floats in LDS beside a 4 KiB exchange area
struct DeconvBwdArgs {
    const float *x, *w, *go;  // x [B,H,W,Cin], w [Cin,Cout/groups,K,K], go [B,stride H,stride W,Cout]
    float *gx, *gw;           // gx nullptr: not computed
    int B, H, W, Cin, Cout, stride, groups;
};
bool cp_deconv_dw_geometry(int Cin, int Cout, int K, int stride, int pad, int groups);
bool cp_deconv_dense_geometry(int Cin, int Cout, int K, int stride, int pad, int groups);
// (for a geometry one of the two predicates accepts)  `precision` (CP_PREC_*): CP_PREC_F16X3 runs the dense layer's two
// contractions in split binary16 -- the weight gradient on conv_bwd16.hip's slab kernel, the data gradient on igemm16.hip where a
// variant takes the launch; the depth-wise layers have no matrix product and are float32 in either mode.
// cp_deconv_backward_prec_mask: bit 0 = the weight gradient, bit 1 = the data gradient runs in f16x3.
size_t cp_deconv_backward_ws_bytes(int B, int H, int W, int Cin, int Cout, int stride, int groups, int need_grad_x, int precision);
int cp_deconv_backward_prec_mask(int B, int H, int W, int Cin, int Cout, int groups, int precision);
int cp_launch_deconv_backward(hipStream_t s, const DeconvBwdArgs& a, void* ws, int precision);

// ---- BatchNorm2d, training and evaluation, fused with the residual add and ReLU (batchnorm.hip): float32 NHWC ----
struct BnFwdArgs {
    const float *x, *gamma, *beta, *res;  // gamma / beta nullptr: 1 / 0; res nullptr: no residual
    float *rmean, *rvar;                  // running statistics: updated (training, may be nullptr) or read (evaluation)
    float *y, *mean, *invstd;
    int B, H, W, C, training;
    float momentum, eps;
    int act;
};
struct BnBwdArgs {
    const float *x, *y, *go, *gamma, *mean, *invstd;  // y (the activated output) or nullptr: grad_out is gated by y > 0
    float *gx, *gres, *gg, *gb;                       // each nullptr: not computed
    int B, H, W, C, training;
};
size_t cp_batchnorm_ws_bytes(int B, int H, int W, int C);
int cp_launch_batchnorm_forward(hipStream_t s, const BnFwdArgs& a, void* ws);
int cp_launch_batchnorm_backward(hipStream_t s, const BnBwdArgs& a, void* ws);
// SyncBatchNorm's four phases (batchnorm.hip); the workspace is cp_batchnorm_ws_bytes'.  BnFwdArgs / BnBwdArgs: `training` is
// not read (always training); mean / invstd are the global pair; gg / gb of the reduce are this rank's own sums.
int cp_batchnorm_sync_rec_floats(int C);
int cp_launch_batchnorm_sync_stats(hipStream_t s, const float* x, float* record, int B, int H, int W, int C, void* ws);
int cp_launch_batchnorm_sync_forward(hipStream_t s, const BnFwdArgs& a, const float* records, int world, float* save_count);
int cp_launch_batchnorm_sync_backward_reduce(hipStream_t s, const BnBwdArgs& a, float* sums, void* ws);
int cp_launch_batchnorm_sync_backward_apply(hipStream_t s, const BnBwdArgs& a, const float* sums_all, int world,
                                            const float* save_count, void* ws);

// ---- GroupNorm for training, fused with the ReLU (groupnorm.hip): float32 NHWC, statistics per (image, group) ----
struct GnFwdArgs {
    const float *x, *gamma, *beta;  // gamma / beta nullptr: 1 / 0
    float *y, *mean, *invstd;       // mean / invstd [B][G]
    int B, H, W, C, G;
    float eps;
    int act;
};
struct GnBwdArgs {
    const float *x, *y, *go, *gamma, *mean, *invstd;  // y (the activated output) or nullptr: grad_out is gated by y > 0
    float *gx, *gg, *gb;                              // each nullptr: not computed
    int B, H, W, C, G;
};
size_t cp_groupnorm_ws_bytes(int B, int H, int W, int C, int G);
int cp_launch_groupnorm_forward(hipStream_t s, const GnFwdArgs& a, void* ws);
int cp_launch_groupnorm_backward(hipStream_t s, const GnBwdArgs& a, void* ws);

// ---- The ConvGRU's gate arithmetic for training (gru_train.hip): x3 / h3 [M][3 Ch], hprev / hout [M][Ch]; h3 nullptr: h = 0 ----
int cp_launch_gru_gate_forward(hipStream_t s, const float* x3, const float* h3, const float* hprev, float* hout, long long M, int Ch);
int cp_launch_gru_gate_backward(hipStream_t s, const float* x3, const float* h3, const float* hprev, const float* go, float* gx3,
                                float* gh3, float* ghp, long long M, int Ch);

// ---- MaxPool2d for training (pool.hip): (kernel, stride, pad) = (2, 2, 0), flooring, or (3, 2, 1), padding as -inf; float32
// NHWC, C % 4 == 0, a non-empty output.  The winner of a window is torch's (first maximum in row-major order) in both calls ----
bool cp_maxpool_geometry(int kernel, int stride, int pad);
int cp_launch_maxpool_forward(hipStream_t s, const float* x, float* out, int B, int H, int W, int C, int kernel);
int cp_launch_maxpool_backward(hipStream_t s, const float* x, const float* go, float* gx, int B, int H, int W, int C, int kernel);

// ---- Weight / bias gradient of the 7x7, padding-3 image stems (stem_bwd.hip): x NCHW with Cin in 1..3 planes, grad_out NHWC ----
struct StemBwdArgs {
    const float *x, *go, *y;  // y (the activated forward output) or nullptr: grad_out is gated by y > 0
    float *gw, *gb;           // gb nullptr: not stored
    int B, H, W, Cin, Cout, stride;
};
// wide: Cout up to 128 (cp_conv2d_stem_wide_backward); otherwise up to 64 (cp_conv2d_stem_backward)
const char* cp_stem_backward_shape_error(int B, int H, int W, int Cin, int Cout, int stride, bool wide = false);  // nullptr: accepted
size_t cp_stem_backward_ws_bytes(int B, int H, int W, int Cin, int Cout, int stride);
int cp_launch_stem_backward(hipStream_t s, const StemBwdArgs& a, void* ws);

// ---- ObjectPoseLoss (pose_loss.hip; numerics in pose_loss_common.h) ----
struct cp_pose_loss_desc;
const char* cp_pose_loss_check(const cp_pose_loss_desc* d);                           // nullptr: accepted
const char* cp_pose_loss_check_grads(const cp_pose_loss_desc* d, const float* const* dmaps,
                                     float* const* grad);  // nullptr: accepted
size_t cp_pose_loss_ws_bytes(const cp_pose_loss_desc* d);                              // 0: refused
int cp_launch_pose_loss_forward(hipStream_t s, const cp_pose_loss_desc* d, float* loss, float* stats, long long* choice,
                                float* terms_out, void* ws);
int cp_launch_pose_loss_backward(hipStream_t s, const cp_pose_loss_desc* d, const float* dloss, const float* const* dmaps,
                                 float* const* grad, void* ws);

// ---- ObjectPose training targets (pose_targets.hip; per-object logic in pose_targets_common.h) ----
struct cp_pose_targets_desc;
const char* cp_pose_targets_check(const cp_pose_targets_desc* d);  // nullptr: accepted (reads the host records)
size_t cp_pose_targets_ws_bytes(const cp_pose_targets_desc* d);    // 0: refused
int cp_launch_pose_targets(hipStream_t s, const cp_pose_targets_desc* d, void* ws);
// ---- the tracking task's targets (pose_targets_track.hip; per-object logic in pose_targets_track_common.h) ----
namespace pose_targets { struct PtTrackCur; }
int cp_launch_pose_targets_cur(hipStream_t s, const cp_pose_targets_desc* d, void* ws, const pose_targets::PtTrackCur* tk);
double* cp_pose_targets_ws_images(const cp_pose_targets_desc* d, void* ws);  // where its launcher stages d->images in `ws`
// the Gaussian map writer of every target builder (pose_targets.hip): each element of each plane written once, as the max
// over the plane's draws that cover it.  A list belongs to (image, channel c): channel 0 draws on out0, 1 + j on outj's joint j.
struct cp_gauss_maps_args {
    float *out0, *outj;   // [images][H][W] and [images][8][H][W], 16-byte aligned; only channels ch0 .. ch0 + nch - 1 are read
    int W, H;             // W * H < 2^31
    int images, nch, ch0;
    int stride;           // list entries per (image, channel): at most 64 without peaks, 128 with
    const int* counts;    // [images * 9]
    const int4* draws;    // [images * 9][stride] (x, y, r, 0)
    const double* peaks;  // [images * 9][stride], or nullptr: every peak is 1
};
size_t cp_gauss_maps_workgroups(size_t planes, size_t plane_elems);  // the grid (the *_check functions hold it below 2^31)
void cp_launch_gauss_maps(hipStream_t s, const cp_gauss_maps_args& a);
struct cp_pose_targets_track_desc;
const char* cp_pose_targets_track_check(const cp_pose_targets_track_desc* d);  // nullptr: accepted
size_t cp_pose_targets_track_ws_bytes(const cp_pose_targets_track_desc* d);    // 0: refused
int cp_launch_pose_targets_track(hipStream_t s, const cp_pose_targets_track_desc* d, void* ws);
// its pieces, for the detector-fed variant (pose_targets_track_det.hip): the staged records and the draw lists inside the
// workspace, the record copies, and everything after the previous-objects kernel
namespace pose_targets { struct PtkOpts; }
struct cp_ptk_ws_view {
    const double *img, *timg, *pre;  // [B][CP_PT_IMG_STRIDE], [B][CP_PTK_IMG_STRIDE], [B][Kp][CP_PTK_PRE_STRIDE]
    void* res;                        // PtkPreOut [B][Kp]
    int* counts;                      // [B * 9]
    void* draws;                      // int4 [B * 9][2 * Kp]
    double* peaks;                    // [B * 9][2 * Kp]
};
pose_targets::PtkOpts cp_ptk_opts(const cp_pose_targets_track_desc* d);
int cp_ptk_stage(hipStream_t s, const cp_pose_targets_track_desc* d, void* ws, cp_ptk_ws_view* v);
int cp_ptk_finish(hipStream_t s, const cp_pose_targets_track_desc* d, void* ws);
// ---- the same with a detector's boxes for some images (pose_targets_track_det.hip; pose_targets_track_det_common.h) ----
struct cp_pose_targets_track_det_desc;
const char* cp_pose_targets_track_det_check(const cp_pose_targets_track_det_desc* d);  // nullptr: accepted
size_t cp_pose_targets_track_det_ws_bytes(const cp_pose_targets_track_det_desc* d);    // 0: refused
int cp_launch_pose_targets_track_det(hipStream_t s, const cp_pose_targets_track_det_desc* d, void* ws);

// ---- training input images (train_inputs.hip; per-pixel arithmetic in train_inputs_common.h) ----
const char* cp_train_inputs_check(const unsigned char* frames, size_t frames_bytes, const double* records, int N,
                                  const float* mean3, const float* std3, const float* out, int out_h,
                                  int out_w);                    // nullptr: accepted (reads the host records)
size_t cp_train_inputs_ws_bytes(int N, int out_h, int out_w);  // 0: refused
int cp_launch_train_inputs(hipStream_t s, const unsigned char* frames, const double* records, int N, const float* mean3,
                           const float* std3, float* out, int out_h, int out_w, void* ws);

// ---- clip + Adam over a param group (optim.hip; table and state layouts in include/centerpose_hip.h) ----
const char* cp_adam_lengths_check(int n_tensors, const int64_t* lengths, const int* active_or_null,
                                  long long* n_chunks);  // nullptr: accepted
size_t cp_adam_table_size(int n_tensors, long long n_chunks);
const char* cp_adam_table_fill(void* table, int n_tensors, const void* const* p, const void* const* g, const void* const* m,
                               const void* const* v, const int64_t* lengths, const int* active_or_null);  // nullptr: written
size_t cp_adam_ws_bytes(int n_chunks);
int cp_launch_adam_step(hipStream_t s, const void* table, int n_tensors, int n_chunks, double lr, double beta1, double beta2, double eps,
                        double weight_decay, double max_norm, int flags, void* state, void* ws);

// ---- the gradient pack of data-parallel training (grad_pack.hip; layouts in include/centerpose_hip.h) ----
const char* cp_grad_layout(int n_tensors, const int64_t* lengths, int64_t* offsets_or_null, long long* flat_elems,
                           long long* n_chunks);  // nullptr: accepted; offsets: n_tensors + 1 values
size_t cp_grad_pack_table_size(int n_tensors, long long n_chunks);
const char* cp_grad_pack_table_fill(void* table, int n_tensors, const void* const* src, const int64_t* lengths,
                                    const int64_t* offsets);  // nullptr: written
long long cp_grad_min_flat_elems(int n_tensors, int n_chunks);
int cp_launch_grad_pack(hipStream_t s, const void* table, int n_tensors, int n_chunks, float* flat, long long flat_elems, float scale);

// ---- Objectron box metrics (box3d.hip; numerics in box3d_common.h) ----
int cp_launch_box_iou(hipStream_t s, const double* a, const double* b, int n, double* iou);
int cp_launch_box_eval(hipStream_t s, const double* pred3d, const double* gt3d, const double* pred2d, const double* mo2c,
                       const double* proj, const int* single, int n, int num_symmetry, double* out);

// ---- batched PnP (pnp.hip) ----
#define CP_PNP_STRIDE 40
size_t cp_pnp_ws_bytes(int N);
int cp_launch_pnp(hipStream_t s, const float* pts, const float* scale, const double* cam, int N, int npts, double* out,
                  void* ws);

int cp_launch_preprocess(const unsigned char* img, int B, int H, int W, const double* trans6, const float* mean3,
                         const float* std3, float* out, int OH, int OW, hipStream_t s);
int cp_launch_resize_u8(const unsigned char* img, int H, int W, int C, unsigned char* out, int OH, int OW, hipStream_t s);

// device post-process + soft-NMS (post.hip); record layout CP_POST_* in include/centerpose_hip.h
int cp_launch_postprocess(const float* det, int B, int K, const double* meta, double vis_thresh, int nms,
                          float div_scale, double* out, int* count, double* ws, hipStream_t s);
int cp_launch_pnp_assemble(const double* post, const int* count, int B, int K, int npts, const double* cam_img, float* pts,
                           float* scale, double* cam, hipStream_t s);
int cp_launch_render_gaussians(const double* recs, int N, float* out, int C, int H, int W, hipStream_t s);

// ---- CenterPoseTrack bookkeeping on the device (track.hip; TrackParams: track_common.h) ----
struct TrackParams;
size_t cp_track_state_bytes_impl(int B, int cap);
size_t cp_track_ws_bytes_impl(int B, int K, int cap);
int cp_launch_track_step(hipStream_t s, const TrackParams& P, const double* vmeta, const double* post, const int* count,
                         const double* det_pnp, int B, int K, void* state, double* recs, void* ws);
int cp_launch_track_seed(hipStream_t s, const TrackParams& P, const double* vmeta, const double* seeds, const int* seed_count,
                         const int* gt_render, int B, int S, void* state, double* recs);
