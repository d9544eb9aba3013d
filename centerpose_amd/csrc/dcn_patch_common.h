// What the patch-resident DCNv2 forward kernels (dcn16p.hip, dcn16s.hip, dcn16t.hip) share, once: the offset / mask record load,
// the bilinear set-up with its exception list, the half-wave exchange, the buffer-load fallback, the blend + split and the
// three-term MFMA group.  dcn16.hip uses dcn_corner_sample for its set-up table.  Each kernel keeps what really differs: staging,
// chunk width and LDS geometry, the K-loop pipeline and weight-set rotation, the lane -> pixel map, the epilogue, the item walk.
//
// The mechanism (dcn_v2_im2col_cuda.cu:25-54, 150-187 is the arithmetic it restates).
//   * A block owns an 8 x 16 patch of output pixels and keeps the input halo of one channel chunk in LDS.  A lane gathers its own
//     MFMA A fragment: pixel = lane % 32, 8 consecutive channels = the 32-byte half lane / 32 of a 16-channel K step.
//   * The bilinear set-up of a lane's 9 taps -- the LDS address of corner (h_lo, w_lo) and 4 corner weights x mask x activation
//     pre-scale per tap -- lives in 45 registers.  The two lanes that share a pixel compute 5 and 4 taps each (dcn_setup_taps:
//     taps 5 lrow .. 5 lrow + 4, slot 4 of the upper half is a dummy) and exchange them by v_permlane32_swap (dcn_expand_taps).
//   * A sample whose 2 x 2 corner block leaves the staged halo is an EXCEPTION: the set-up appends (key, global offset, 4 weights)
//     to the block's list (LDS atomic) and takes weights (1, 0, 0, 0) on spare pixel e itself; the kernel's staging blends the four
//     corners per chunk into that spare pixel, which the K loop then reads like any other corner -- no branch.  The spare pixels
//     and the three zero-weight "corners" next to the last one are zeroed by the kernel.
//   * A block with more exceptions than its capacity switches, as a whole, to gathering through buffer loads like dcn16.hip
//     (slower, same results): dcn_setup_global rebuilds corner offset | 4 validity bits + weights from the whole record (the fast
//     set-up does not keep the offsets, and it replaced the weights of the samples it filed), dcn_gather_global loads the corners
//     with the invalid ones sent out of range (-> 0).
//   * Blend: fma(w4, v4, fma(w3, v3, fma(w2, v2, w1 * v1))) per channel, plain v_fma_f32 (dcn16.hip's order; its packed form
//     measured 4 % slower beside MFMAs, MI355X_MICROARCH.md), then split2 into binary16 hi / lo.  MFMA terms in igemm16.hip's
//     order: lo * hi, hi * lo, hi * hi.
// Everything here is a transcription of code that sits exactly on the kernels' register budgets (tests/test_upadd_epilogue_cpu.py):
// expression order, asm statements and wait states are part of the contract.
#pragma once
#include "igemm16_common.h"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// buf_ld4 with a scalar (wave-uniform) byte offset on top of the per-lane one
__device__ __forceinline__ float4 buf_ld4s(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// both 32-lane halves of `v` for every lane: {lower half's value, upper half's value}
__device__ __forceinline__ void both_halves5(const uint32_t (&v)[5], uint32_t (&lo)[5], uint32_t (&hi)[5]) {
    // v_permlane32_swap_b32 vdst, vsrc exchanges vdst[32..63] with vsrc[0..31]; with both operands holding v every lane ends up
    // with {the lower half's value, the upper half's value}.  Written out by hand, each swap on its own pair of registers with
    // the wait states the hazard table asks for inside the statement (VALU write -> v_permlane*_swap read: 2).  (Round 4 padded
    // these swaps while hunting wrong set-up values; the swaps were innocent -- the cause was a packed-f32 op with a set op_sel
    // bit, profiles/NOTES.md round 5 -- but the hand-written form costs nothing and stays.)
    uint32_t a0 = v[0], a1 = v[1], a2 = v[2], a3 = v[3], a4 = v[4], b0 = v[0], b1 = v[1], b2 = v[2], b3 = v[3], b4 = v[4];
    asm volatile("s_nop 4\n\tv_permlane32_swap_b32 %0, %5\n\ts_nop 1\n\tv_permlane32_swap_b32 %1, %6\n\ts_nop 1\n\t"
                 "v_permlane32_swap_b32 %2, %7\n\ts_nop 1\n\tv_permlane32_swap_b32 %3, %8\n\ts_nop 1\n\t"
                 "v_permlane32_swap_b32 %4, %9\n\ts_nop 4"
                 : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3), "+v"(b4));
    lo[0] = a0; lo[1] = a1; lo[2] = a2; lo[3] = a3; lo[4] = a4;
    hi[0] = b0; hi[1] = b1; hi[2] = b2; hi[3] = b3; hi[4] = b4;
}

// A lane (or thread) id the compiler cannot see through: what is derived from it is rebuilt where it is used (a handful of VALU)
// instead of being hoisted and held -- or spilled -- across the K loops.
__device__ __forceinline__ int lane_opaque(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

// This lane's share of its pixel's offset / mask record (32 floats at byte `rec`: 18 offsets, 9 masks): taps 5 lrow .. 5 lrow + 4
__device__ __forceinline__ void dcn_load_record(__amdgpu_buffer_rsrc_t r_om, unsigned rec, int lrow, float (&od)[12], float (&omk)[5]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float4 v = buf_ld4(r_om, rec + (unsigned)lrow * 40u + 16u * i);
        od[4 * i] = v.x; od[4 * i + 1] = v.y; od[4 * i + 2] = v.z; od[4 * i + 3] = v.w;
    }
    const float4 v = buf_ld4(r_om, rec + 72u + (unsigned)lrow * 20u);
    omk[0] = v.x; omk[1] = v.y; omk[2] = v.z; omk[3] = v.w;
    omk[4] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r_om, (int)(rec + 88u + (unsigned)lrow * 20u), 0, 0));
}

// A block's exception list (LDS): per sample, the key (h_lo + 1) << 16 | (w_lo + 1) of its top-left corner, that corner's byte
// offset into the input tensor (may be "before" it: the key gives the corners' validity), its four corner weights; the counter.
struct DcnExcList {
    int* key;
    int* goff;
    float* w;  // [capacity][4], 16-byte aligned
    int* count;
};

// Set-up of the lane's five tap slots for the pixel (b, y, x) of the patch whose top-left output pixel is (ty0, tx0).  G is the
// kernel's LDS geometry: PH x PW staged pixels around the patch with HALO on every side, ECAP exception samples, and what sq[]
// counts in -- G::corner(qy, qx) of staged pixel (qy, qx), G::spare(e) of spare pixel e.  sw[][]: weights x mask x pre-scale.
template <class G>
__device__ __forceinline__ void dcn_setup_taps(const float (&od)[12], const float (&omk)[5], int lrow, int y, int x, int ty0,
                                               int tx0, int b, int H, int W, int cb, float afwd, const DcnExcList& exc,
                                               uint32_t (&sq)[5], uint32_t (&sw)[5][4]) {
    const float fy0 = (float)(y - 1), fx0 = (float)(x - 1);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        // tap 5 lrow + j = (kh, kw): lower half (0,0) (0,1) (0,2) (1,0) (1,1); upper half (1,2) (2,0) (2,1) (2,2) (-)
        const float khf = lrow ? (float)((5 + j) / 3) : (float)(j / 3);
        const float kwf = lrow ? (float)((5 + j) % 3) : (float)(j % 3);
        float h_im = (fy0 + khf) + od[2 * j];
        float w_im = (fx0 + kwf) + od[2 * j + 1];
        const bool valid = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W && !(lrow && j == 4);
        h_im = valid ? h_im : 0.f;  // keeps the arithmetic below finite; its weights are zeroed through the mask
        w_im = valid ? w_im : 0.f;
        const float mk = valid ? omk[j] * afwd : 0.f;
        const float fh = floorf(h_im), fw = floorf(w_im);
        const int h_lo = (int)fh, w_lo = (int)fw;
        const float lh = h_im - fh, lw = w_im - fw;
        const float hh = 1.f - lh, hw = 1.f - lw;
        sw[j][0] = __float_as_uint(hh * hw * mk);
        sw[j][1] = __float_as_uint(hh * lw * mk);
        sw[j][2] = __float_as_uint(lh * hw * mk);
        sw[j][3] = __float_as_uint(lh * lw * mk);
        const int qy = h_lo - (ty0 - G::HALO), qx = w_lo - (tx0 - G::HALO);
        const bool inp = (unsigned)qy <= (unsigned)(G::PH - 2) && (unsigned)qx <= (unsigned)(G::PW - 2);
        int q = inp ? G::corner(qy, qx) : 0;
        if (valid && !inp) {  // exception sample: file its corner and weights; the staging blends it into spare pixel e,
                              // which this lane then reads with weights (1, 0, 0, 0)
            const int e = atomicAdd(exc.count, 1);
            if (e < G::ECAP) {
                exc.key[e] = ((h_lo + 1) << 16) | (w_lo + 1);
                exc.goff[e] = ((b * H + h_lo) * W + w_lo) * cb;
                *reinterpret_cast<float4*>(exc.w + 4 * e) = make_float4(__uint_as_float(sw[j][0]), __uint_as_float(sw[j][1]),
                                                                        __uint_as_float(sw[j][2]), __uint_as_float(sw[j][3]));
                sw[j][0] = __float_as_uint(1.f);
                sw[j][1] = sw[j][2] = sw[j][3] = 0u;
                q = G::spare(e);
            }
        }
        sq[j] = (uint32_t)q;
    }
}

// Both halves swap their five slots: addr[t] = sq of tap t x QB bytes + this lane's 32-byte channel half, bw[t] = {w1, w2}, {w3, w4}
template <int QB>
__device__ __forceinline__ void dcn_expand_taps(const uint32_t (&sq)[5], const uint32_t (&sw)[5][4], int lrow, int (&addr)[9],
                                                f32x2 (&bw)[9][2]) {
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const uint32_t pack[5] = {sq[j], sw[j][0], sw[j][1], sw[j][2], sw[j][3]};
        uint32_t lo[5], hi[5];
        both_halves5(pack, lo, hi);
        addr[j] = (int)lo[0] * QB + lrow * 32;
        if (j < 4) addr[5 + j] = (int)hi[0] * QB + lrow * 32;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            bw[j][c >> 1][c & 1] = __uint_as_float(lo[1 + c]);
            if (j < 4) bw[5 + j][c >> 1][c & 1] = __uint_as_float(hi[1 + c]);
        }
    }
}

// One sample at (h_im, w_im) of image b, mk = mask x activation pre-scale: byte offset of corner (h_lo, w_lo) into the input tensor
// with the 4 corner-validity bits in its low bits (the offset is a multiple of cb = Cin * 4 >= 128; it may be "before" the tensor
// when h_lo / w_lo = -1: only valid corners are ever dereferenced), and the 4 corner weights.  All zeros outside the image.
struct DcnCorner {
    int base;
    float w1, w2, w3, w4;
};
__device__ __forceinline__ DcnCorner dcn_corner_sample(float h_im, float w_im, float mk, int b, int H, int W, int cb) {
    DcnCorner r = {0, 0.f, 0.f, 0.f, 0.f};
    if (h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W) {
        const int h_lo = (int)floorf(h_im), w_lo = (int)floorf(w_im);
        const float lh = h_im - (float)h_lo, lw = w_im - (float)w_lo;
        const float hh = 1.f - lh, hw = 1.f - lw;
        int vm = 0;
        if (h_lo >= 0 && w_lo >= 0) vm |= 1;
        if (h_lo >= 0 && w_lo + 1 <= W - 1) vm |= 2;
        if (h_lo + 1 <= H - 1 && w_lo >= 0) vm |= 4;
        if (h_lo + 1 <= H - 1 && w_lo + 1 <= W - 1) vm |= 8;
        r.base = (((b * H + h_lo) * W + w_lo) * cb) | vm;
        r.w1 = hh * hw * mk; r.w2 = hh * lw * mk; r.w3 = lh * hw * mk; r.w4 = lh * lw * mk;
    }
    return r;
}

// Buffer-load mode: corner offset | validity bits and the weights of all 9 taps of pixel (b, y, x), from the whole record
__device__ __forceinline__ void dcn_setup_global(__amdgpu_buffer_rsrc_t r_om, unsigned rec, int y, int x, int b, int H, int W, int cb,
                                                 float afwd, int (&addr)[9], f32x2 (&bw)[9][2]) {
    float o9[28];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const float4 v = buf_ld4(r_om, rec + 16u * i);
        o9[4 * i] = v.x; o9[4 * i + 1] = v.y; o9[4 * i + 2] = v.z; o9[4 * i + 3] = v.w;
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float h_im = (float)(y - 1 + t / 3) + o9[2 * t];
        const float w_im = (float)(x - 1 + t % 3) + o9[2 * t + 1];
        const DcnCorner s = dcn_corner_sample(h_im, w_im, o9[18 + t] * afwd, b, H, W, cb);
        addr[t] = s.base;
        bw[t][0] = f32x2{s.w1, s.w2};
        bw[t][1] = f32x2{s.w3, s.w4};
    }
}

// ... and one K step's gather: the 4 corners of a = addr[tap], this lane's two channel quads, + scalar channel offset `so`
__device__ __forceinline__ void dcn_gather_global(__amdgpu_buffer_rsrc_t r_x, int a, int lrow, int rowb, int cb, int so,
                                                  float4 (&r)[4][2]) {
    const int base = (a & ~15) + lrow * 32;
#pragma unroll
    for (int c = 0; c < 4; ++c) {  // invalid corners out of range (-> 0)
        const int gi = (a & (1 << c)) ? base + (c >> 1) * rowb + (c & 1) * cb : (int)OOB_BASE;
        r[c][0] = buf_ld4s(r_x, (unsigned)gi, so);
        r[c][1] = buf_ld4s(r_x, (unsigned)gi + 16u, so);
    }
}

__device__ __forceinline__ float4 dcn_blend4(float w1, float w2, float w3, float w4, const float4& v1, const float4& v2,
                                             const float4& v3, const float4& v4) {
    float4 o;
    o.x = fmaf(w4, v4.x, fmaf(w3, v3.x, fmaf(w2, v2.x, w1 * v1.x)));
    o.y = fmaf(w4, v4.y, fmaf(w3, v3.y, fmaf(w2, v2.y, w1 * v1.y)));
    o.z = fmaf(w4, v4.z, fmaf(w3, v3.z, fmaf(w2, v2.z, w1 * v1.z)));
    o.w = fmaf(w4, v4.w, fmaf(w3, v3.w, fmaf(w2, v2.w, w1 * v1.w)));
    return o;
}

// Staging of a chunk's exception samples (dcn16p, dcn16t: 256 threads, Q = the chunk's channel quads per pixel): Q threads per
// sample, 256 / Q samples per pass.  The four corners (validity from the key) are blended here into spare pixel e, PSTR bytes
// apart from `spare`; addresses are rebuilt per chunk from the block's list -- no registers held across the K loop.
template <int Q, int PSTR>
__device__ __forceinline__ void dcn_stage_exceptions(int t, int nexc, const DcnExcList& exc, __amdgpu_buffer_rsrc_t r_x, int H, int W,
                                                     int cb, int rowb, int csoff, unsigned char* spare) {
    static_assert(Q == 4 || Q == 8, "16 or 32 channels per chunk");
    constexpr int QS = Q == 8 ? 3 : 2;
    for (int e = t >> QS; e < nexc; e += 256 / Q) {
        const int key = exc.key[e], go = exc.goff[e] + (t & (Q - 1)) * 16;
        const float4 w = *reinterpret_cast<const float4*>(exc.w + 4 * e);
        const int iy = (key >> 16) - 1, ix = (key & 0xffff) - 1;
        const bool y0 = (unsigned)iy < (unsigned)H, y1 = (unsigned)(iy + 1) < (unsigned)H;
        const bool x0 = (unsigned)ix < (unsigned)W, x1 = (unsigned)(ix + 1) < (unsigned)W;
        const float4 v1 = buf_ld4s(r_x, (y0 && x0) ? (unsigned)go : OOB, csoff);
        const float4 v2 = buf_ld4s(r_x, (y0 && x1) ? (unsigned)(go + cb) : OOB, csoff);
        const float4 v3 = buf_ld4s(r_x, (y1 && x0) ? (unsigned)(go + rowb) : OOB, csoff);
        const float4 v4 = buf_ld4s(r_x, (y1 && x1) ? (unsigned)(go + rowb + cb) : OOB, csoff);
        *reinterpret_cast<float4*>(spare + e * PSTR + (t & (Q - 1)) * 16) = dcn_blend4(w.x, w.y, w.z, w.w, v1, v2, v3, v4);
    }
}

// Blend + split of one gathered K step (r[corner][quad], w = {w1, w2}, {w3, w4}) into the binary16 hi / lo A operands
__device__ __forceinline__ void dcn_blend_split(const float4 (&r)[4][2], const f32x2 (&w)[2], h8* ah, h8* al) {
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int hq = 0; hq < 2; ++hq) {
        const float4 o = dcn_blend4(w[0].x, w[0].y, w[1].x, w[1].y, r[0][hq], r[1][hq], r[2][hq], r[3][hq]);
        const Split2 t0 = split2(o.x, o.y), t1 = split2(o.z, o.w);
        hi[2 * hq] = t0.hi; hi[2 * hq + 1] = t1.hi;
        lo[2 * hq] = t0.lo; lo[2 * hq + 1] = t1.lo;
    }
    const u32x4 ahv = {hi[0], hi[1], hi[2], hi[3]}, alv = {lo[0], lo[1], lo[2], lo[3]};
    *ah = *reinterpret_cast<const h8*>(&ahv);
    *al = *reinterpret_cast<const h8*>(&alv);
}

// The step's 3 N MFMAs.  TRANSPOSED: weights as the first operand -- the accumulators hold the transposed tile (rows = output
// channels, columns = this wave's pixels): accumulator 4 g + i of N tile j in lane (pixel lane % 32, half h4) = channel
// 32 j + 8 g + 4 h4 + i of that pixel, so the epilogue stores 16 bytes at a time.
template <bool TRANSPOSED, int N>
__device__ __forceinline__ void dcn_mma3(Frag<32>::acc_t* acc, const h8& ah, const h8& al, const u32x4 (&bh)[N], const u32x4 (&bl)[N]) {
    auto mfma = [&](int j, const h8& a, const u32x4& bw) {
        const h8 b = *reinterpret_cast<const h8*>(&bw);
        if constexpr (TRANSPOSED) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b, a, acc[j], 0, 0, 0);
        else acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[j], 0, 0, 0);
    };
#pragma unroll
    for (int j = 0; j < N; ++j) mfma(j, al, bh[j]);
#pragma unroll
    for (int j = 0; j < N; ++j) mfma(j, ah, bl[j]);
#pragma unroll
    for (int j = 0; j < N; ++j) mfma(j, ah, bh[j]);
}

}  // namespace
