// The f16x3 forms of the Conv2d backward's two MFMA contractions (conv_bwd.hip; CP_CONV_BWD_MFMA geometries): every float32
// operand is pre-scaled by an exact power of two, split into two binary16 numbers hi + lo (split2: hi rounded towards zero,
// lo = the rounded residual) and each product block is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with float32
// accumulation -- the arithmetic of the forward's CP_PREC_F16X3 kernels (igemm16.hip, deconv16.hip).  Only the matrix-core sums
// change: the gate, the pad lanes and grad_bias stay stage_kernel's float32.  No atomics but the |max| slots'; every sum has a
// fixed order.
//
// Operands.  A split tensor is stored as one dword per element, binary16 hi in the low half and lo in the high half
// (split_kernel): the same four bytes as the float32 element, so every load keeps the float32 kernels' memory shape, and a
// fragment of eight elements becomes its two MFMA operands with eight v_perm_b32.
//   gs16   grad_out, gated and padded (conv_bwd.hip's gs), times 2^e_g from its |max| slot
//   x16    x times 2^e_x from its |max| slot (weight gradient; 1x1 layers have none: wgrad16_kernel splits x in registers)
//   w      times 2^e_c per INPUT channel c (a row of the data gradient's GEMM), 2^-e_c in w_inv
//            stride 1: [cpad][taps CoP] binary16 hi / lo, taps mirrored and channel roles swapped: igemm16.hip's operand
//            stride 2: wT16 [tap][CoP][Cin] split dwords
// Kernels.
//   wgrad16_kernel     slab[s][co][k] as wgrad_kernel, sixteen output pixels per MFMA step: a lane owns one channel (lane & 31)
//                      and eight consecutive pixels (lane >> 5 selects which eight), so every load is still a whole 128-byte
//                      line per half-wave.  The step after the one in the matrix core is always in flight (two fragment sets,
//                      loop unrolled by two: no register copies); rows are walked as one flat sequence of steps, so the
//                      prefetch crosses row ends.  2^-(e_g + e_x) is applied by wgrad_reduce_kernel (conv_bwd.hip).
//   dgrad16_s2_kernel  dgrad_s2_kernel's parity classes, tap lists and stores; K steps of sixteen CoP lanes.
//   stride 1           cp_launch_conv16 on gs (float32, in_amax = gs's slot) with the packed weight.
#include "op_common.h"
#include "igemm16_common.h"

#include <algorithm>

namespace {

// max |x[0..n)| into `slot` (any alignment)
__global__ __launch_bounds__(256) void absmax32_kernel(const float* __restrict__ x, size_t n, unsigned* __restrict__ slot) {
    float m = 0.f;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) m = fmaxf(m, fabsf(x[i]));
    cp_amax_commit(slot, m);
}

// dst[i] = split(src[i] * 2^e), e from the slot
__global__ __launch_bounds__(256) void split_kernel(const float* __restrict__ src, uint32_t* __restrict__ dst, size_t n,
                                                    const unsigned* __restrict__ slot) {
    float fwd, inv;
    cp_amax_to_scale(cp_amax_read(slot), &fwd, &inv);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = split_dword(src[i] * fwd);
}

template <int NH>
struct WFrag {
    uint32_t a[NH][8], b[2][8];
};

// slab[s][co][k], wgrad_kernel's jobs (a wave: NH co tiles x 2 k tiles) and slab layout.  A[co][q] = gs16[q][h0 + lane & 31],
// B[q][k] = x16[q * stride + tap - pad][c0 + lane & 31], q = the step's pixel 8 (lane >> 5) + j; out-of-image taps, the ragged
// end of a row and the steps past the slab's end are zeros by select on clamped addresses.  XF: `x` is the float32 tensor itself
// and the B fragment is scaled and split in registers (split2 on pairs gives the operand dwords directly: the same bits as the
// split copy) -- for 1x1 layers, which read every x element exactly once, so a split copy would only add two passes over x.
template <int NH, bool XF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void wgrad16_kernel(
    const uint32_t* __restrict__ gs, const uint32_t* __restrict__ x, const unsigned* __restrict__ x_amax, float* __restrict__ slab,
    int rows, int Ho, int Wo, int H, int W, int Cin, int CoP, int KW, int taps, int stride, int pad, int rows_per_slab) {
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
    float xf = 1.f, xi = 1.f;
    if (XF) cp_amax_to_scale(cp_amax_read(x_amax), &xf, &xi);
    // the cursor of the next step to request (wave-uniform): output row, its image and line, first pixel of the step
    int row = row_beg, cb = row_beg / Ho, coy = row_beg - cb * Ho, x0 = 0;
    auto load = [&](WFrag<NH>& f) {
        const bool rv = row < row_end;
        const int rw = rv ? row : row_beg;
        const uint32_t* arow = gs + (size_t)rw * Wo * CoP + h0 + r;
        const uint32_t* brow[2];
        bool yv[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int iy = coy * stride + dy[n];
            yv[n] = rv && kv[n] && (unsigned)iy < (unsigned)H;
            brow[n] = x + ((size_t)cb * H + (yv[n] ? iy : 0)) * W * Cin + c0[n] + r;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ox = x0 + 8 * hh + j;
            const bool xv = rv && ox < Wo;
            const int xc = xv ? ox : 0;
#pragma unroll
            for (int t = 0; t < NH; ++t) {
                const uint32_t v = arow[(size_t)xc * CoP + 32 * t];
                f.a[t][j] = xv ? v : 0u;
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int ix = ox * stride + dx[n];
                const bool ok = xv && yv[n] && (unsigned)ix < (unsigned)W;
                const uint32_t v = brow[n][(size_t)(ok ? ix : 0) * Cin];
                f.b[n][j] = ok ? v : 0u;
            }
        }
        // advance (past the slab's end the cursor stays on its last image: rv is false from then on)
        x0 += 16;
        if (x0 >= Wo && rv) {
            x0 = 0;
            ++row;
            if (++coy == Ho && row < row_end) {
                coy = 0;
                ++cb;
            }
        }
    };
    auto mma = [&](const WFrag<NH>& f) {
        h8 ah[NH], al[NH], bh[2], bl[2];
#pragma unroll
        for (int t = 0; t < NH; ++t) unpack8(f.a[t], ah[t], al[t]);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            if (XF) {
                u32x4 h, l;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const Split2 sp = split2(__uint_as_float(f.b[n][2 * k]) * xf, __uint_as_float(f.b[n][2 * k + 1]) * xf);
                    h[k] = sp.hi;
                    l[k] = sp.lo;
                }
                bh[n] = __builtin_bit_cast(h8, h);
                bl[n] = __builtin_bit_cast(h8, l);
            } else {
                unpack8(f.b[n], bh[n], bl[n]);
            }
        }
#pragma unroll
        for (int t = 0; t < NH; ++t)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[t][n] = mma3(ah[t], al[t], bh[n], bl[n], acc[t][n]);
    };
    const int total = (row_end - row_beg) * ((Wo + 15) / 16);
    WFrag<NH> f0, f1;
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
                out[(size_t)h * TC + k] = acc[t][n][e];
            }
        }
}

// (2^e, 2^-e) per input channel c of w [Cout][Cin][taps]: max over (co, tap) |w| * 2^e in [2^14, 2^15); all-zero channels: 1
__global__ __launch_bounds__(64) void wscale_cin_kernel(const float* __restrict__ w, int Cout, int Cin, int taps, float* __restrict__ fwd,
                                                        float* __restrict__ inv) {
    const int c = blockIdx.x, n = Cout * taps;
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) {
        const int co = i / taps, t = i - co * taps;
        m = fmaxf(m, fabsf(w[((size_t)co * Cin + c) * taps + t]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if (threadIdx.x == 0) {
        float f = 1.f, iv = 1.f;
        if (m > 0.f) cp_amax_to_scale(__float_as_uint(m), &f, &iv);
        fwd[c] = f;
        inv[c] = iv;
    }
}

// The data gradient's weight operand from w [Cout][Cin][taps] times fwd[c] (buffers pre-zeroed: pad rows stay zero).
// wT == nullptr (stride 1): hi / lo [c][(taps - 1 - tap) * CoP + co], rows of Kpad16 halfs; else (stride 2) wT[tap][co][c].
__global__ void pack_dgrad16_kernel(const float* __restrict__ w, const float* __restrict__ fwd, uint16_t* __restrict__ hi,
                                    uint16_t* __restrict__ lo, uint32_t* __restrict__ wT, int Cout, int CoP, int Cin, int taps) {
    const size_t n = (size_t)Cout * Cin * taps, Kpad16 = (size_t)taps * CoP;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int co = (int)(e / ((size_t)Cin * taps));
        const int rr = (int)(e - (size_t)co * Cin * taps), c = rr / taps, t = rr - c * taps;
        const uint32_t d = split_dword(w[e] * fwd[c]);
        if (wT) {
            wT[((size_t)t * CoP + co) * Cin + c] = d;
        } else {
            const size_t o = (size_t)c * Kpad16 + (size_t)(taps - 1 - t) * CoP + co;
            hi[o] = (uint16_t)(d & 0xffffu);
            lo[o] = (uint16_t)(d >> 16);
        }
    }
}

// dgrad_s2_kernel on the split operands: the same parity classes, tap lists, M tiles and stores.  A[pixel][k]: a lane reads
// the 32 bytes k0 + 8 (lane >> 5) .. + 8 of its pixel's gs16 row; B[k][c] = wT16[tap][k][n0 + lane & 31]: a 128-byte line per
// half and k.  The epilogue undoes the two pre-scales: acc * 2^-e_g * 2^-e_c.
template <int NT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void dgrad16_s2_kernel(
    const uint32_t* __restrict__ gs, const uint32_t* __restrict__ wT, float* __restrict__ gx, const unsigned* __restrict__ g_amax,
    const float* __restrict__ w_inv, int B, int H, int W, int Cin, int CoP, int Ho, int Wo, int KK, int pad) {
    constexpr int DU = 2;
    __shared__ int opix[4][64];
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int py = blockIdx.y >> 1, px = blockIdx.y & 1;
    const int Hc = (H - py + 1) >> 1, Wc = (W - px + 1) >> 1, M = B * Hc * Wc;
    const int NG = Cin / (32 * NT);
    const int job = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
    const int mt = job / NG, ng = job - mt * NG;
    const bool active = mt * 64 < M;  // wave-uniform
    const int n0 = ng * 32 * NT;
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
            const uint32_t* ap[2];
            bool ok[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int oy = pjy[i] + oyo, ox = pjx[i] + oxo;
                ok[i] = pv[i] && (unsigned)oy < (unsigned)Ho && (unsigned)ox < (unsigned)Wo;
                ap[i] = gs + (ok[i] ? (((size_t)pb[i] * Ho + oy) * Wo + ox) * CoP : 0) + 8 * hh;
            }
            const uint32_t* bp = wT + (size_t)(ky * KK + kx) * CoP * Cin + (size_t)(8 * hh) * Cin + n0 + r;
            auto load = [&](int k0, uint32_t (&a)[2][8], uint32_t (&bq)[NT][8]) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const u32x4 v0 = *reinterpret_cast<const u32x4*>(ap[i] + k0), v1 = *reinterpret_cast<const u32x4*>(ap[i] + k0 + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        a[i][j] = ok[i] ? v0[j] : 0u;
                        a[i][4 + j] = ok[i] ? v1[j] : 0u;
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j)
#pragma unroll
                    for (int t = 0; t < NT; ++t) bq[t][j] = bp[(size_t)(k0 + j) * Cin + 32 * t];
            };
            // DU steps of sixteen k per chunk, all requested before the chunk's first MFMA (CoP % 32 == 0: whole chunks)
            for (int k0 = 0; k0 < CoP; k0 += 16 * DU) {
                uint32_t a[DU][2][8], bq[DU][NT][8];
#pragma unroll
                for (int u = 0; u < DU; ++u) load(k0 + 16 * u, a[u], bq[u]);
#pragma unroll
                for (int u = 0; u < DU; ++u) {
                    h8 ah[2], al[2], bh[NT], bl[NT];
#pragma unroll
                    for (int i = 0; i < 2; ++i) unpack8(a[u][i], ah[i], al[i]);
#pragma unroll
                    for (int t = 0; t < NT; ++t) unpack8(bq[u][t], bh[t], bl[t]);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int t = 0; t < NT; ++t) acc[i][t] = mma3(ah[i], al[i], bh[t], bl[t], acc[i][t]);
                }
            }
        }
    }
    float gf, gi, wi[NT];
    cp_amax_to_scale(cp_amax_read(g_amax), &gf, &gi);
#pragma unroll
    for (int t = 0; t < NT; ++t) wi[t] = w_inv[n0 + r + 32 * t];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int o = opix[wv][i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh];
            if (o < 0) continue;
            float* dst = gx + (size_t)o * Cin + n0 + r;
#pragma unroll
            for (int t = 0; t < NT; ++t) dst[32 * t] = cp_scale_pow2(acc[i][t][e], gi, wi[t]);
        }
}

inline int nh16_of(int c) { return c % 64 == 0 ? 2 : 1; }

// N tile padding of the stride-1 data gradient's convolution (its outputs are the layer's Cin input channels)
inline size_t dgrad16_cpad(int Cin) { return cp_engine::align_up((size_t)Cin, cp_conv_tile_n(Cin)); }

// the packed weight's regions inside the caller's buffer
struct Dgrad16Ws {
    float *fwd, *inv;
    void *hi, *lo, *fhi, *flo;
    uint32_t* wT;
};
Dgrad16Ws dgrad16_carve(Carve& c, int Cin, int CoP, int taps, int stride) {
    const size_t cpad = dgrad16_cpad(Cin), halfs = stride == 1 ? cpad * taps * CoP * 2 : 0;
    Dgrad16Ws r;
    r.fwd = c.take<float>(cpad * 4);
    r.inv = c.take<float>(cpad * 4);
    r.hi = c.take<void>(halfs);
    r.lo = c.take<void>(halfs);
    r.fhi = c.take<void>(halfs);
    r.flo = c.take<void>(halfs);
    r.wT = c.take<uint32_t>(stride == 1 ? 0 : (size_t)taps * CoP * Cin * 4);
    return r;
}

ConvParams dgrad16_s1_params(const ConvBwdArgs& a, const float* gs, int CoP, const Dgrad16Ws& r, const float* res, const unsigned* gs_amax) {
    ConvParams d = grad_conv_params(a.B, a.H, a.W, gs, CoP, nullptr, nullptr, a.Cin, a.KH, a.KW, 1, a.pad, a.gx);
    d.res = res;
    d.res_ld = a.Cin;
    d.w16_hi = r.hi;
    d.w16_lo = r.lo;
    d.w16f_hi = r.fhi;
    d.w16f_lo = r.flo;
    d.Kpad16 = a.KH * a.KW * CoP;
    d.scale = r.inv;
    d.in_amax[0] = gs_amax;
    return d;
}

}  // namespace

int cp_launch_absmax32(const float* x, size_t n, unsigned* slot, hipStream_t s) {
    const size_t g = std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 2048));
    hipLaunchKernelGGL(absmax32_kernel, dim3((unsigned)g), dim3(256), 0, s, x, n, slot);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_split16(const float* src, uint32_t* dst, size_t n, const unsigned* slot, hipStream_t s) {
    const size_t g = std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 8192));
    hipLaunchKernelGGL(split_kernel, dim3((unsigned)g), dim3(256), 0, s, src, dst, n, slot);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_conv_wgrad16_slabs(hipStream_t s, const ConvBwdArgs& a, const ConvWgrad16& h, int CoP, const ConvWgradPlan& P, float* slab) {
    const int Ho = (a.H + 2 * a.pad - a.KH) / a.stride + 1, Wo = (a.W + 2 * a.pad - a.KW) / a.stride + 1;
    const int taps = a.KH * a.KW, rows = a.B * Ho, slabs = (rows + P.rows_per_slab - 1) / P.rows_per_slab;
    const int nh = nh16_of(CoP), KT = taps * a.Cin / 32, jobs = (CoP / (32 * nh)) * ((KT + 1) / 2);
    const dim3 wg((jobs + 3) / 4, 1, slabs);
    // (no split copy of x: the kernel splits a.x, read as its bits, in registers)
    const uint32_t* xb = h.x16 ? h.x16 : reinterpret_cast<const uint32_t*>(a.x);
#define CP_WGRAD16(NH, XF)                                                                                                        \
    hipLaunchKernelGGL((wgrad16_kernel<NH, XF>), wg, dim3(256), 0, s, h.gs16, xb, h.x_amax, slab, rows, Ho, Wo, a.H, a.W, a.Cin, CoP, \
                       a.KW, taps, a.stride, a.pad, P.rows_per_slab)
    if (nh == 2 && h.x16) CP_WGRAD16(2, false);
    else if (nh == 2) CP_WGRAD16(2, true);
    else if (h.x16) CP_WGRAD16(1, false);
    else CP_WGRAD16(1, true);
#undef CP_WGRAD16
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

size_t cp_conv_dgrad16_pack_bytes(int Cin, int CoP, int taps, int stride) {
    Carve c{nullptr};
    dgrad16_carve(c, Cin, CoP, taps, stride);
    return c.off;
}

int cp_launch_conv_dgrad16_pack(hipStream_t s, const float* w, void* wB, int Cin, int Cout, int CoP, int taps, int stride) {
    Carve c{(char*)wB};
    const Dgrad16Ws r = dgrad16_carve(c, Cin, CoP, taps, stride);
    if (hipMemsetAsync(wB, 0, c.off, s) != hipSuccess) return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(wscale_cin_kernel, dim3(Cin), dim3(64), 0, s, w, Cout, Cin, taps, r.fwd, r.inv);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    const size_t n = (size_t)Cout * Cin * taps;
    hipLaunchKernelGGL(pack_dgrad16_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, w,
                       (const float*)r.fwd, (uint16_t*)r.hi, (uint16_t*)r.lo, stride == 1 ? (uint32_t*)nullptr : r.wT, Cout, CoP, Cin, taps);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    if (stride != 1) return CP_OK;
    const int cpad = (int)dgrad16_cpad(Cin), Kpad16 = taps * CoP;
    const int rc = cp_launch_frag16_repack(r.hi, r.fhi, cpad, Kpad16, s);
    return rc != CP_OK ? rc : cp_launch_frag16_repack(r.lo, r.flo, cpad, Kpad16, s);
}

bool cp_conv_dgrad16_s1_supported(int B, int H, int W, int Cin, int CoP, int K) {
    // (host arithmetic on the launch's shape: the pointers only have to be there)
    static const float dummy = 0.f;
    const ConvBwdArgs a{&dummy, &dummy, nullptr, &dummy, nullptr, nullptr, nullptr, B, H, W, Cin, CoP, K, K, 1, K / 2};
    Dgrad16Ws r{};
    r.hi = r.lo = (void*)&dummy;
    return cp_conv16_supported(dgrad16_s1_params(a, &dummy, CoP, r, nullptr, nullptr));
}

int cp_launch_conv_dgrad16_s1(hipStream_t s, const ConvBwdArgs& a, const float* gs, int CoP, const void* wB, const float* res,
                              const unsigned* gs_amax) {
    Carve c{(char*)wB};
    const Dgrad16Ws r = dgrad16_carve(c, a.Cin, CoP, a.KH * a.KW, 1);
    return cp_launch_conv16(dgrad16_s1_params(a, gs, CoP, r, res, gs_amax), s);
}

int cp_launch_conv_dgrad16_s2(hipStream_t s, const ConvBwdArgs& a, const uint32_t* gs16, int CoP, const void* wB, const unsigned* gs_amax) {
    Carve c{(char*)wB};
    const Dgrad16Ws r = dgrad16_carve(c, a.Cin, CoP, a.KH * a.KW, 2);
    const int Ho = (a.H + 2 * a.pad - a.KH) / 2 + 1, Wo = (a.W + 2 * a.pad - a.KW) / 2 + 1;
    const int M0 = a.B * ((a.H + 1) / 2) * ((a.W + 1) / 2);  // the even / even class has the most pixels
    const int nt = nh16_of(a.Cin), jobs = ((M0 + 63) / 64) * (a.Cin / (32 * nt));
    const dim3 dg((jobs + 3) / 4, 4);
#define CP_DGRAD16(NT)                                                                                                          \
    hipLaunchKernelGGL(dgrad16_s2_kernel<NT>, dg, dim3(256), 0, s, gs16, (const uint32_t*)r.wT, a.gx, gs_amax, (const float*)r.inv, \
                       a.B, a.H, a.W, a.Cin, CoP, Ho, Wo, a.KH, a.pad)
    if (nt == 2) CP_DGRAD16(2);
    else CP_DGRAD16(1);
#undef CP_DGRAD16
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
