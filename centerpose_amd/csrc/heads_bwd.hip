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
//   3. wgrad    slab[s][h][k] = sum over the pixel rows of slab s of grad_hidden[q][h] * feat[q + tap][c], k = tap * Cin + c
//               (wgrad0_kernel: v_mfma_f32_32x32x2_f32 with K = pixels, operands straight from global memory, a wave owns
//               NH x 2 accumulators); wgrad0_reduce_kernel sums the slabs in slab order into the PyTorch layout;
//   4. dgrad    grad_feat (+)= grad_hidden (*) flipped w0^T: the same implicit GEMM with K = 9 hid; the first head writes
//               the chunk, later heads add to it through the kernel's residual input (same stream: no atomics, no halo
//               exchange).  Skipped entirely when the caller passes no grad_feat.
//   grad_b1 = per-channel sums of grad_out in a fixed tree (rowsum_kernel), once per head.
// Every sum has a fixed order, so all outputs are bitwise reproducible run to run.  The hidden chunk makes one round trip
// through memory per step (write in 1, read + write in 2, read in 3 and 4): 16 MiB per image and head at 128 x 128 x 256
// against 14.5 GFLOP of contractions, i.e. a few percent of the matrix time; it is the price of building steps 1 and 4
// from the library's tuned convolution instead of a hand-fused tile pipeline.
#include "igemm_common.h"

#include <algorithm>
#include <cstring>

namespace {

constexpr size_t kChunkBytes = (size_t)256 << 20;  // the recomputed hidden chunk (dcn_bwd.hip's grad_col precedent)
constexpr int TL = 1024;                           // floats of one wave's grad_out tile in LDS (thin_kernel)

// wB[(8 - tap) * hid + h][c] = w0[h][c][tap]: the data gradient is the 3x3 / pad 1 convolution of grad_hidden with the
// taps mirrored and the channel roles swapped
__global__ void pack_dgrad_kernel(const float* __restrict__ w0, float* __restrict__ wB, int hid, int Cin, int cpad) {
    const size_t n = (size_t)hid * Cin * 9;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const int h = (int)(e / ((size_t)Cin * 9));
        const int r = (int)(e - (size_t)h * Cin * 9), c = r / 9, t = r - c * 9;
        wB[((size_t)(8 - t) * hid + h) * cpad + c] = w0[e];
    }
}

// One pass over the hidden chunk hb [Q][hid] (pre-activation in, grad_hidden out).  A workgroup owns `slab_px` pixels and 64
// hidden channels (lane = channel); its four waves take tiles of PT pixels in turn.  go_t [Q][cls] is the chunk's grad_out
// pixel-major; a wave stages its tile in LDS (zero-padded to CMAX channels) and reads it back as broadcasts.
// part[slab][c][h], c < cls: grad_w1 partial; c == cls: grad_b0 partial.  Sums: pixels ascending per wave, then waves 0..3.
template <int CMAX>
__global__ __launch_bounds__(256) void thin_kernel(float* __restrict__ hb, const float* __restrict__ go_t,
                                                   const float* __restrict__ w1, float* __restrict__ part, int Q, int hid,
                                                   int cls, int slab_px) {
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
    float gb0 = 0.f;
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
                const float a = fmaxf(v[u], 0.f);
                float g = 0.f;
                const float* gr = &gs[wv][(j0 + u) * CMAX];
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    const float gc = gr[c];
                    acc[c] = fmaf(a, gc, acc[c]);
                    g = fmaf(gc, w1r[c], g);
                }
                g = v[u] > 0.f ? g : 0.f;
                if (hv) hb[(size_t)(qb + j0 + u) * hid + h] = g;
                gb0 += g;
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
    if (!hv) return;
    float* out = part + (size_t)blockIdx.x * (cls + 1) * hid;
    for (int c = wv; c <= cls; c += 4) out[(size_t)c * hid + h] = red[(c < cls ? c : CMAX) * 64 + lane];
}

// gw1[c][h] and gb0[h] = (accum ? previous : 0) + the slabs' partials in slab order
__global__ void thin_reduce_kernel(const float* __restrict__ part, float* __restrict__ gw1, float* __restrict__ gb0, int nslab,
                                   int cls, int hid, int accum) {
    const int n = (cls + 1) * hid;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        float* dst = e < cls * hid ? gw1 + e : gb0 + (e - cls * hid);
        float v = accum ? *dst : 0.f;
        for (int s = 0; s < nslab; ++s) v += part[(size_t)s * n + e];
        *dst = v;
    }
}

// slab[s][h][k] over the image rows [s * rows_per_slab, ...) of the chunk: D[h][k] with K = pixels, two per MFMA step (lane
// half = pixel parity along x).  A[h][q] = gh[q][h0 + lane & 31] (a 128-byte line per half), B[q][k] = feat[q + tap][c0 +
// lane & 31] (likewise: a k tile of 32 stays inside one tap because Cin % 32 == 0); out-of-image taps and the ragged last
// pixel of an odd row are zeros by select, never by a branch around the load.  A wave owns NH h tiles x 2 k tiles; the four
// waves of a workgroup take neighbouring k tile pairs of the same h tiles.
template <int NH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void wgrad0_kernel(const float* __restrict__ gh, const float* __restrict__ feat,
                                                     float* __restrict__ slab, int rows, int H, int W, int Cin, int hid,
                                                     int rows_per_slab) {
    const int TC = 9 * Cin, KT = TC / 32, KJ = (KT + 1) / 2;
    const int lane = threadIdx.x & 63, r = lane & 31, hh = lane >> 5;
    const int job = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const int hg = job / KJ, kj = job - hg * KJ;
    if (hg * 32 * NH >= hid) return;
    const int h0 = hg * 32 * NH;
    int dy[2], dx[2], c0[2];
    bool kv[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int kt = kj * 2 + n;
        kv[n] = kt < KT;
        const int k0 = kv[n] ? kt * 32 : 0, tap = k0 / Cin;
        c0[n] = k0 - tap * Cin;
        dy[n] = tap / 3 - 1;
        dx[n] = tap - (tap / 3) * 3 - 1;
    }
    f32x16 acc[NH][2];
#pragma unroll
    for (int t = 0; t < NH; ++t)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][n][e] = 0.f;
    const int row_beg = blockIdx.z * rows_per_slab, row_end = min(rows, row_beg + rows_per_slab);
    for (int row = row_beg; row < row_end; ++row) {
        const int y = row % H;
        const float* arow = gh + (size_t)row * W * hid + h0 + r;
        const float* brow[2];
        bool yv[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            yv[n] = kv[n] && (unsigned)(y + dy[n]) < (unsigned)H;
            brow[n] = feat + (size_t)(yv[n] ? row + dy[n] : row) * W * Cin + c0[n] + r;
        }
        // two pixels per step; the next step's operands are loaded before this step's MFMAs are issued
        auto load = [&](int x0, float (&a)[NH], float (&b)[2]) {
            const int x = x0 + hh;
            const bool xv = x < W;
            const int xc = xv ? x : W - 1;
#pragma unroll
            for (int t = 0; t < NH; ++t) {
                const float v = arow[(size_t)xc * hid + 32 * t];
                a[t] = xv ? v : 0.f;
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int xx = x + dx[n];
                const bool ok = xv && yv[n] && (unsigned)xx < (unsigned)W;
                const float v = brow[n][(size_t)(ok ? xx : xc) * Cin];
                b[n] = ok ? v : 0.f;
            }
        };
        float a[NH], b[2], an[NH], bn[2];
        load(0, a, b);
        for (int x0 = 0; x0 < W; x0 += 2) {
            load(x0 + 2, an, bn);  // (past the row's end: clamped addresses, zeros)
#pragma unroll
            for (int t = 0; t < NH; ++t)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[t][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b[n], acc[t][n], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NH; ++t) a[t] = an[t];
            b[0] = bn[0];
            b[1] = bn[1];
        }
    }
    float* out = slab + (size_t)blockIdx.z * hid * TC;
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

// grad_w0[h][c][tap] = (accum ? previous : 0) + the slabs [h][tap * Cin + c] in slab order
__global__ void wgrad0_reduce_kernel(const float* __restrict__ slab, float* __restrict__ gw, int nslab, int hid, int Cin,
                                     int accum) {
    const size_t TC = (size_t)9 * Cin, n = (size_t)hid * TC;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t h = e / TC;
        const int r = (int)(e - h * TC), c = r / 9, t = r - c * 9;
        const size_t src = h * TC + (size_t)t * Cin + c;
        float v = accum ? gw[e] : 0.f;
        for (int s = 0; s < nslab; ++s) v += slab[(size_t)s * n + src];
        gw[e] = v;
    }
}

// gb[c] = sum over images and pixels of g [B][C][HW]: a fixed per-thread stride and a fixed tree
__global__ __launch_bounds__(256) void rowsum_kernel(const float* __restrict__ g, float* __restrict__ gb, int B, int C, int HW) {
    __shared__ float red[256];
    const int c = blockIdx.x;
    float v = 0.f;
    for (int b = 0; b < B; ++b) {
        const float* pl = g + ((size_t)b * C + c) * HW;
        for (int e = threadIdx.x; e < HW; e += 256) v += pl[e];
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) gb[c] = red[0];
}

inline size_t al(size_t x) { return (x + 255) / 256 * 256; }
inline bool ok() { return hipGetLastError() == hipSuccess; }
inline int nh_of(int hid) { return hid % 128 == 0 ? 4 : hid % 64 == 0 ? 2 : 1; }

struct Plan {
    int nb;                           // images per chunk
    int hpad, cpad;                   // hid / Cin padded to their convolution's N tile
    int thin_px, thin_slabs;          // thin_kernel: pixels per slab, slabs of a full chunk
    int wg_rows, wg_slabs, wg_jobs;   // wgrad0_kernel: image rows per slab, slabs of a full chunk, wave jobs
    size_t wA, wB, shift, hb, go_t, part, slab, total;  // byte offsets / total
};

Plan plan(int B, int H, int W, int Cin, int hid, int cmax) {
    Plan P;
    const size_t HW = (size_t)H * W;
    P.nb = cp_pose_heads_chunk(B, H, W, hid);
    P.hpad = (int)((hid + cp_conv_tile_n(hid) - 1) / cp_conv_tile_n(hid) * cp_conv_tile_n(hid));
    P.cpad = (int)((Cin + cp_conv_tile_n(Cin) - 1) / cp_conv_tile_n(Cin) * cp_conv_tile_n(Cin));
    const size_t Q = (size_t)P.nb * HW;
    // thin: about two workgroups per CU and channel group, at least 256 pixels a slab
    size_t ts = std::max<size_t>(1, std::min<size_t>(512, (Q + 255) / 256));
    P.thin_px = (int)((Q + ts - 1) / ts);
    P.thin_slabs = (int)((Q + P.thin_px - 1) / P.thin_px);
    // wgrad: about two waves per SIMD; slabs of whole image rows, at most 64 MiB of them
    const int KT = 9 * Cin / 32;
    P.wg_jobs = (hid / (32 * nh_of(hid))) * ((KT + 1) / 2);
    const size_t rows = (size_t)P.nb * H;
    size_t ns = (2048 + P.wg_jobs - 1) / P.wg_jobs;
    ns = std::min(ns, std::max<size_t>(1, ((size_t)64 << 20) / ((size_t)hid * 9 * Cin * 4)));
    ns = std::max<size_t>(1, std::min(ns, rows));
    P.wg_rows = (int)((rows + ns - 1) / ns);
    P.wg_slabs = (int)((rows + P.wg_rows - 1) / P.wg_rows);
    size_t o = 0;
    P.wA = o;
    o += al((size_t)9 * Cin * P.hpad * 4);
    P.wB = o;
    o += al((size_t)9 * hid * P.cpad * 4);
    P.shift = o;
    o += al((size_t)P.hpad * 4);
    P.hb = o;
    o += al(Q * hid * 4);
    P.go_t = o;
    o += al(Q * cmax * 4);
    P.part = o;
    o += al((size_t)P.thin_slabs * (cmax + 1) * hid * 4);
    P.slab = o;
    o += al((size_t)P.wg_slabs * hid * 9 * Cin * 4);
    P.total = o;
    return P;
}

}  // namespace

int cp_pose_heads_chunk(int B, int H, int W, int hid) {
    const size_t per_img = (size_t)H * W * hid * 4;
    const size_t cap = std::min<size_t>(kChunkBytes / per_img, 16384);  // (the layout kernels put the chunk's images on grid z)
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)B, cap));
}

size_t cp_pose_heads_backward_ws_bytes(int B, int H, int W, int Cin, int hid, int max_classes) {
    return plan(B, H, W, Cin, hid, max_classes).total;
}

int cp_launch_pose_heads_backward(hipStream_t s, const PoseHeadsArgs& a, const float* const* grad_out, float* const* grad_w0,
                                  float* const* grad_b0, float* const* grad_w1, float* const* grad_b1, float* grad_feat,
                                  void* ws) {
    int cmax = 1;
    for (int i = 0; i < a.n; ++i) cmax = std::max(cmax, a.classes[i]);
    const Plan P = plan(a.B, a.H, a.W, a.Cin, a.hid, cmax);
    char* w8 = (char*)ws;
    float* wA = (float*)(w8 + P.wA);
    float* wB = (float*)(w8 + P.wB);
    float* shift = (float*)(w8 + P.shift);
    float* hb = (float*)(w8 + P.hb);
    float* go_t = (float*)(w8 + P.go_t);
    float* part = (float*)(w8 + P.part);
    float* slab = (float*)(w8 + P.slab);
    const int B = a.B, H = a.H, W = a.W, Cin = a.Cin, hid = a.hid, HW = H * W;
    bool feat_written = false;
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
        // the head's packed operands: wA [9 Cin][hpad] and b0 padded for the hidden layer, wB [9 hid][cpad] for the data gradient
        if (hipMemsetAsync(wA, 0, P.hb - P.wA, s) != hipSuccess) return CP_ERR_LAUNCH;
        int rc = cp_launch_pack_weight(a.w0[i], wA, hid, Cin, 9, Cin, P.hpad, 0, s);
        if (rc != CP_OK) return rc;
        if (hipMemcpyAsync(shift, a.b0[i], (size_t)hid * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return CP_ERR_LAUNCH;
        if (grad_feat) {
            hipLaunchKernelGGL(pack_dgrad_kernel, dim3(256), dim3(256), 0, s, a.w0[i], wB, hid, Cin, P.cpad);
            if (!ok()) return CP_ERR_LAUNCH;
        }
        hipLaunchKernelGGL(rowsum_kernel, dim3(cls), dim3(256), 0, s, grad_out[i], grad_b1[i], B, cls, HW);
        if (!ok()) return CP_ERR_LAUNCH;
        for (int b0 = 0; b0 < B; b0 += P.nb) {
            const int nb = std::min(P.nb, B - b0), Q = nb * HW, accum = b0 > 0;
            const float* fc = a.feat + (size_t)b0 * HW * Cin;
            // 1. hidden (pre-activation)
            ConvParams p;
            memset(&p, 0, sizeof(p));
            p.nsrc = 1;
            p.src[0] = fc;
            p.src_c[0] = p.Cin = Cin;
            p.B = nb, p.H = p.Ho = H, p.W = p.Wo = W;
            p.KH = p.KW = 3, p.stride = 1, p.pad = 1;
            p.K = p.Kpad = 9 * Cin;
            p.wp = wA;
            p.Cout = hid, p.CoutPad = P.hpad;
            p.shift = shift;
            p.act = CP_ACT_NONE;
            p.out = hb;
            p.store = CP_STORE_NHWC;
            p.ldo = hid;
            rc = cp_launch_conv(p, s);
            if (rc != CP_OK) return rc;
            // 2. thin
            rc = cp_launch_nchw_to_nhwc(grad_out[i] + (size_t)b0 * cls * HW, go_t, nb, cls, H, W, cls, s);
            if (rc != CP_OK) return rc;
            const int tslabs = (Q + P.thin_px - 1) / P.thin_px;
            const dim3 tg(tslabs, (hid + 63) / 64);
            if (cls <= 4)
                hipLaunchKernelGGL(thin_kernel<4>, tg, dim3(256), 0, s, hb, (const float*)go_t, a.w1[i], part, Q, hid, cls, P.thin_px);
            else if (cls <= 16)
                hipLaunchKernelGGL(thin_kernel<16>, tg, dim3(256), 0, s, hb, (const float*)go_t, a.w1[i], part, Q, hid, cls, P.thin_px);
            else
                hipLaunchKernelGGL(thin_kernel<64>, tg, dim3(256), 0, s, hb, (const float*)go_t, a.w1[i], part, Q, hid, cls, P.thin_px);
            if (!ok()) return CP_ERR_LAUNCH;
            hipLaunchKernelGGL(thin_reduce_kernel, dim3(((cls + 1) * hid + 255) / 256), dim3(256), 0, s, (const float*)part,
                               grad_w1[i], grad_b0[i], tslabs, cls, hid, accum);
            if (!ok()) return CP_ERR_LAUNCH;
            // 3. grad_w0
            const int rows = nb * H, wslabs = (rows + P.wg_rows - 1) / P.wg_rows;
            const dim3 wg((P.wg_jobs + 3) / 4, 1, wslabs);
            switch (nh_of(hid)) {
                case 4: hipLaunchKernelGGL(wgrad0_kernel<4>, wg, dim3(256), 0, s, (const float*)hb, fc, slab, rows, H, W, Cin, hid, P.wg_rows); break;
                case 2: hipLaunchKernelGGL(wgrad0_kernel<2>, wg, dim3(256), 0, s, (const float*)hb, fc, slab, rows, H, W, Cin, hid, P.wg_rows); break;
                default: hipLaunchKernelGGL(wgrad0_kernel<1>, wg, dim3(256), 0, s, (const float*)hb, fc, slab, rows, H, W, Cin, hid, P.wg_rows);
            }
            if (!ok()) return CP_ERR_LAUNCH;
            hipLaunchKernelGGL(wgrad0_reduce_kernel, dim3(576), dim3(256), 0, s, (const float*)slab, grad_w0[i], wslabs, hid, Cin,
                               accum);
            if (!ok()) return CP_ERR_LAUNCH;
            // 4. grad_feat of the chunk: written by the first head with a gradient, added to by the others
            if (grad_feat) {
                float* gf = grad_feat + (size_t)b0 * HW * Cin;
                ConvParams d;
                memset(&d, 0, sizeof(d));
                d.nsrc = 1;
                d.src[0] = hb;
                d.src_c[0] = d.Cin = hid;
                d.B = nb, d.H = d.Ho = H, d.W = d.Wo = W;
                d.KH = d.KW = 3, d.stride = 1, d.pad = 1;
                d.K = d.Kpad = 9 * hid;
                d.wp = wB;
                d.Cout = Cin, d.CoutPad = P.cpad;
                d.act = CP_ACT_NONE;
                d.res = feat_written ? gf : nullptr;
                d.res_ld = Cin;
                d.out = gf;
                d.store = CP_STORE_NHWC;
                d.ldo = Cin;
                rc = cp_launch_conv(d, s);
                if (rc != CP_OK) return rc;
            }
        }
        feat_written = true;
    }
    if (grad_feat && !feat_written && hipMemsetAsync(grad_feat, 0, (size_t)B * HW * Cin * 4, s) != hipSuccess) return CP_ERR_LAUNCH;
    return CP_OK;
}
