// Dense ConvTranspose2d(Cin, Cout, k=4, stride=2, pad=1) + folded BatchNorm + optional ReLU as one implicit GEMM per output
// parity class (resnet_dcn.py: PoseResNet._make_deconv_layer's `up` layers, followed by BatchNorm2d and ReLU).
//
// Sub-pixel form: output pixel (2i + py, 2j + px) only receives the input rows iy = i + py - 1 + ty and columns
// ix = j + px - 1 + tx (ty, tx in {0, 1}) through taps ky = 3 - py - 2 ty, kx = 3 - px - 2 tx.  Each of the four classes
// (py, px) is therefore a stride-1 2x2 convolution over the input grid: M = B*H*W rows, N = Cout, K = 4*Cin with
// k = (2 ty + tx) * Cin + ci.  blockIdx.z is the class; every class writes straight into the interleaved NHWC output.
//
// Both precisions run the same register-only stream (no LDS): a wave owns a 64 x 64 tile (2 x 2 MFMA fragments of 32 x 32)
// and loads its operands with raw buffer loads, one K step of 32 ahead of the matrix instructions.  Within a K step lane
// half q = lane >> 5 holds channels [16q, 16q + 16) of its pixel: 64 contiguous bytes per lane, the two halves together
// one whole 128-byte line per pixel.  A and B use the same k permutation, so the contraction is unchanged.
//   f32    16 x v_mfma_f32_32x32x2_f32 per fragment and step, weights as float32 [class][CoutPad][K]
//   f16x3   2 x 3 x v_mfma_f32_32x32x16_f16 (hi*hi + hi*lo + lo*hi), weights pre-split as binary16 [class][CoutPad][K]
//          hi / lo with a power-of-two scale per output channel; the activations are scaled by 2^e_a from the input's |max|
//          slot before the split (ConvParams::in_amax) and the output's |max| goes to its slot.
// Halo taps and rows past M read through an out-of-range buffer offset (zeros), so the loop has no branches.
#include "igemm16_common.h"

namespace {

constexpr int DC_WAVES = 4;         // waves per workgroup, stacked along M
constexpr int DC_BM = 64 * DC_WAVES;  // rows of a workgroup tile
constexpr int DC_BN = 64;           // output channels of a workgroup tile

struct DeconvArgs {
    const float* x;      // [B,H,W,Cin]
    const void* w;       // f32: float [4][CoutPad][K]; f16x3: binary16 hi [4][CoutPad][K]
    const void* w_lo;    // f16x3: binary16 lo, same layout
    const float* scale;  // [CoutPad] (f16x3: already times 2^-e_w) or nullptr
    const float* shift;  // [CoutPad] or nullptr
    float* out;          // [B,2H,2W,Cout]
    const unsigned* in_amax;
    unsigned* out_amax;
    int B, H, W, Cin, Cout, CoutPad, relu;
};

// (b, i, j) of the input-grid row m and the byte offsets of its four taps for class (py, px) (OOB_BASE when outside)
__device__ __forceinline__ void tap_offsets(const DeconvArgs& a, const PixelDecomp& pd, int m, int M, int py, int px,
                                            unsigned (&o)[4]) {
    int b, i, j;
    pd.split(m < M ? m : 0, &b, &i, &j);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int iy = i + py - 1 + (t >> 1), ix = j + px - 1 + (t & 1);
        const bool ok = m < M && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        o[t] = ok ? (unsigned)((((size_t)b * a.H + iy) * a.W + ix) * a.Cin) * 4u : OOB_BASE;
    }
}

template <bool F16>
__global__ void __launch_bounds__(64 * DC_WAVES) deconv_kernel(DeconvArgs a) {
    typedef Frag<32> F;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cls = blockIdx.z, py = cls >> 1, px = cls & 1;
    const int M = a.B * a.H * a.W, K = 4 * a.Cin, csteps = a.Cin / 32;
    const int mw = blockIdx.x * DC_BM + wv * 64;  // first row of this wave
    const int n0 = blockIdx.y * DC_BN;
    const int row = lane & 31, q = lane >> 5;
    PixelDecomp pd;
    pd.init(a.H, a.W, M);
    unsigned off[2][4];
    tap_offsets(a, pd, mw + row, M, py, px, off[0]);
    tap_offsets(a, pd, mw + 32 + row, M, py, px, off[1]);
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x, (unsigned)((size_t)M * a.Cin * 4));
    float afwd = 1.f, ainv = 1.f;
    if (F16 && a.in_amax) cp_amax_to_scale(cp_amax_read(a.in_amax), &afwd, &ainv);

    // weights: lane (col, q) reads row n0 + 32 jn + col, k = 32 s + 16 q .. + 16
    const size_t wcls = (size_t)cls * a.CoutPad * K;
    const int esz = F16 ? 2 : 4;
    const __amdgpu_buffer_rsrc_t rw = make_rsrc((const char*)a.w + wcls * esz, (unsigned)((size_t)a.CoutPad * K * esz));
    const __amdgpu_buffer_rsrc_t rwl = make_rsrc((const char*)(F16 ? a.w_lo : a.w) + wcls * esz, (unsigned)((size_t)a.CoutPad * K * esz));
    unsigned woff[2];
#pragma unroll
    for (int jn = 0; jn < 2; ++jn) woff[jn] = (unsigned)(((size_t)(n0 + 32 * jn + row) * K + 16 * q) * esz);

    F::acc_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // operand registers of one K step: A 2 fragments x 16 floats, B 2 fragments x (f32: 16 floats; f16x3: 8 + 8 dwords)
    float4 ra[2][4];
    u32x4 rb[2][4];
    // operands of K step (tap t, channel chunk c); t is a compile-time index at every call, so no select on it
    auto load = [&](int t, int c, float4 (&A)[2][4], u32x4 (&Bv)[2][4]) {
        const int s = t * csteps + c;
        const unsigned co = (unsigned)(c * 32 + 16 * q) * 4u;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned base = off[i][t] + co;
#pragma unroll
            for (int c = 0; c < 4; ++c) A[i][c] = buf_ld4(rx, base + 16u * c);
        }
        const unsigned kb = (unsigned)(s * 32 * esz);
#pragma unroll
        for (int jn = 0; jn < 2; ++jn) {
            if (F16) {
                Bv[jn][0] = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(woff[jn] + kb), 0, 0);
                Bv[jn][1] = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(woff[jn] + kb + 16), 0, 0);
                Bv[jn][2] = __builtin_amdgcn_raw_buffer_load_b128(rwl, (int)(woff[jn] + kb), 0, 0);
                Bv[jn][3] = __builtin_amdgcn_raw_buffer_load_b128(rwl, (int)(woff[jn] + kb + 16), 0, 0);
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c) Bv[jn][c] = __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(woff[jn] + kb + 16 * c), 0, 0);
            }
        }
    };
    auto compute = [&](const float4 (&A)[2][4], const u32x4 (&Bv)[2][4]) {
        if constexpr (F16) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {  // channels 16q + 8h .. + 8
                h8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const float4 u = A[i][2 * h], v = A[i][2 * h + 1];
                    const Split2 s0 = split2(u.x * afwd, u.y * afwd), s1 = split2(u.z * afwd, u.w * afwd);
                    const Split2 s2 = split2(v.x * afwd, v.y * afwd), s3 = split2(v.z * afwd, v.w * afwd);
                    const u32x4 hv = {s0.hi, s1.hi, s2.hi, s3.hi}, lv = {s0.lo, s1.lo, s2.lo, s3.lo};
                    ah[i] = __builtin_bit_cast(h8, hv);
                    al[i] = __builtin_bit_cast(h8, lv);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    bh[j] = __builtin_bit_cast(h8, Bv[j][h]);
                    bl[j] = __builtin_bit_cast(h8, Bv[j][2 + h]);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                    }
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float av[2], bv[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const float4 u = A[i][c];
                        av[i] = e == 0 ? u.x : e == 1 ? u.y : e == 2 ? u.z : u.w;
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) bv[j] = __uint_as_float(Bv[j][c][e]);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][j] = F::mfma(av[i], bv[j], acc[i][j]);
                }
            }
        }
    };

    // one K step: prefetch (tn, cn) into registers, run the matrix instructions on the current operands, rotate
    auto step = [&](int tn, int cn) {
        float4 na[2][4];
        u32x4 nb[2][4];
        // the phase order is pinned (sched_barrier): left alone, the scheduler sinks every load of step n + 1 below the
        // matrix instructions of step n and the next step waits for the full L2 round trip (vmcnt(0) after 4 MFMAs)
        load(tn, cn, na, nb);
        __builtin_amdgcn_sched_barrier(0);
        compute(ra, rb);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                ra[i][c] = na[i][c];
                rb[i][c] = nb[i][c];
            }
    };
    load(0, 0, ra, rb);
    // taps unrolled, channel chunks a counted loop; each tap's last step prefetches the next tap's first chunk (the very last
    // step re-reads its own operands, which are never used): no branch and no select in the stream
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        for (int c = 0; c + 1 < csteps; ++c) step(t, c + 1);
        step(t < 3 ? t + 1 : 3, t < 3 ? 0 : csteps - 1);
    }

    // epilogue: y = acc * scale * 2^-e_a + shift (+ ReLU) -> out[b, 2i + py, 2j + px, n]; 32 lanes store one 128-byte line
    const int Wo = 2 * a.W;
    float amax = 0.f;
    const __amdgpu_buffer_rsrc_t ro = make_rsrc(a.out, (unsigned)((size_t)M * 4 * a.Cout * 4));
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + 32 * j + row;
        const bool n_ok = n < a.Cout;  // scale / shift are read below Cout only (stand-alone callers pass [Cout] arrays)
        const float sc = (n_ok && a.scale ? a.scale[n] : 1.f) * ainv, sh = n_ok && a.shift ? a.shift[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mw + 32 * i + F::row(r, lane);
                float v = acc[i][j][r] * sc + sh;
                if (a.relu) v = cp_relu(v);
                int b, ii, jj;
                pd.split(m < M ? m : 0, &b, &ii, &jj);
                const bool ok = n_ok && m < M;
                if (ok) amax = fmaxf(amax, fabsf(v));
                const unsigned o = ok ? (unsigned)(((((size_t)b * 2 * a.H + 2 * ii + py) * Wo + 2 * jj + px) * a.Cout + n) * 4)
                                      : OOB;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, (int)o, 0, 0);
            }
        }
    }
    if (a.out_amax) cp_amax_commit(a.out_amax + 0, amax);
}

// PyTorch ConvTranspose2d weight [Cin][Cout][4][4] -> the four classes' sub-kernels [class][CoutPad][K] (rows >= Cout zero).
// f16x3: per output channel co a power of two 2^e (max |w[:, co]| * 2^e in [2^14, 2^15)), hi / lo split of w * 2^e, inv[co] = 2^-e.
__global__ void deconv_pack_kernel(const float* __restrict__ w, float* __restrict__ wf, _Float16* __restrict__ hi,
                                   _Float16* __restrict__ lo, float* __restrict__ inv, int Cin, int Cout, int CoutPad) {
    const int co = blockIdx.x, K = 4 * Cin;
    float mx = 0.f;
    if (co < Cout)
        for (int i = threadIdx.x; i < Cin * 16; i += 64) mx = fmaxf(mx, fabsf(w[((size_t)(i >> 4) * Cout + co) * 16 + (i & 15)]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float f = 1.f, iv = 1.f;
    if (mx > 0.f) cp_amax_to_scale(__float_as_uint(mx), &f, &iv);
    if (inv && threadIdx.x == 0) inv[co] = iv;
    // e walks [ci][ky][kx] of this output channel: 16 consecutive floats of the source per input channel
    for (int e = threadIdx.x; e < 16 * Cin; e += 64) {
        const int ci = e >> 4, ky = (e >> 2) & 3, kx = e & 3;
        const int py = (3 - ky) & 1, ty = (3 - ky) >> 1, px = (3 - kx) & 1, tx = (3 - kx) >> 1;  // ky = 3 - py - 2 ty
        const int cls = 2 * py + px, k = (2 * ty + tx) * Cin + ci;
        const float v = co < Cout ? w[((size_t)ci * Cout + co) * 16 + ky * 4 + kx] : 0.f;
        const size_t d = ((size_t)cls * CoutPad + co) * K + k;
        if (wf) wf[d] = v;
        if (hi) {
            const float x = v * f;
            const _Float16 h = (_Float16)x;  // round to nearest; the residual carries the rest
            hi[d] = h;
            lo[d] = (_Float16)(x - (float)h);
        }
    }
}

}  // namespace

int cp_deconv_cout_pad(int Cout) { return (Cout + DC_BN - 1) / DC_BN * DC_BN; }

int cp_launch_pack_deconv(const float* w, float* wf, void* hi, void* lo, float* inv, int Cin, int Cout, hipStream_t s) {
    if (Cin % 32 || Cout <= 0) return CP_ERR_INVALID;
    hipLaunchKernelGGL(deconv_pack_kernel, dim3(cp_deconv_cout_pad(Cout)), dim3(64), 0, s, w, wf, (_Float16*)hi, (_Float16*)lo, inv, Cin,
                       Cout, cp_deconv_cout_pad(Cout));
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_deconv(const DeconvLaunch& l, hipStream_t s) {
    if (l.Cin % 32 || l.Cout <= 0 || l.B <= 0 || l.H <= 0 || l.W <= 0) return CP_ERR_INVALID;
    const size_t M = (size_t)l.B * l.H * l.W, CoutPad = (size_t)cp_deconv_cout_pad(l.Cout);
    // 32-bit buffer offsets: input, output and one class of weights must stay below the OOB_BASE sentinel
    if (M * l.Cin * 4 >= OOB_BASE || M * 4 * l.Cout * 4 >= OOB_BASE || CoutPad * 4 * l.Cin * 4 >= OOB_BASE) return CP_ERR_INVALID;
    DeconvArgs a;
    a.x = l.x;
    a.w = l.f16x3 ? l.w_hi : l.wf;
    a.w_lo = l.w_lo;
    a.scale = l.scale;
    a.shift = l.shift;
    a.out = l.out;
    a.in_amax = l.f16x3 ? l.in_amax : nullptr;
    a.out_amax = l.out_amax;
    a.B = l.B;
    a.H = l.H;
    a.W = l.W;
    a.Cin = l.Cin;
    a.Cout = l.Cout;
    a.CoutPad = (int)CoutPad;
    a.relu = l.relu;
    if (!a.w || (l.f16x3 && !a.w_lo)) return CP_ERR_INVALID;
    const dim3 grid((unsigned)((M + DC_BM - 1) / DC_BM), (unsigned)(CoutPad / DC_BN), 4);
    if (l.f16x3) hipLaunchKernelGGL(deconv_kernel<true>, grid, dim3(64 * DC_WAVES), 0, s, a);
    else hipLaunchKernelGGL(deconv_kernel<false>, grid, dim3(64 * DC_WAVES), 0, s, a);
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}
