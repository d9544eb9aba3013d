// The ConvGRU's gate arithmetic for training (cp_gru_gate_forward / cp_gru_gate_backward): ConvGRUCell.forward of
// convGRU.py:32-39 after its six convolutions, and autograd's gradients of it, each in one pass.
//   x3 = [Wir x + b | Wiz x + b | Win x + b] and h3 = [Whr h | Whz h | Whn h] as [M][3 Ch], hprev / hout [M][Ch], float32:
//   r = sigmoid(x3r + h3r), z = sigmoid(x3z + h3z), n = tanh(x3n + r h3n), hout = (1 - z) n + z hprev.
// h3 == nullptr is step 0 of every forward: h = 0 and, the hidden-side convolutions having no bias, h3 = 0.
// The backward recomputes r, z and n from its inputs: no gate tensor is kept between the calls.
// A lane owns four channels of one row and moves 16 bytes per access; Ch / 4 neighbouring lanes cover a row's run of each
// tensor (Ch = 64: 256 bytes, whole 128-byte lines).  Forward 8 Ch floats per row (7 in, 1 out), backward 15 Ch (8 in, 7 out);
// at step 0 4 Ch and 7 Ch.  expf / tanhf as the engine's inference kernel (ewise.hip): the results are compared with float64.
#include "op_common.h"
#include "igemm_common.h"

namespace {

__device__ __forceinline__ float sigm(float a) { return 1.f / (1.f + expf(-a)); }

struct Gate {
    float r, z, n;
};
__device__ __forceinline__ Gate gate(float xr, float xz, float xn, float hr, float hz, float hn) {
    Gate g;
    g.r = sigm(xr + hr);
    g.z = sigm(xz + hz);
    g.n = tanhf(fmaf(g.r, hn, xn));
    return g;
}

__device__ __forceinline__ void un(const float4 v, float (&o)[4]) { o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w; }
__device__ __forceinline__ void st(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }

// one thread per (row, four channels); items = M * Ch / 4
__global__ __launch_bounds__(256) void gate_fwd_kernel(const float* __restrict__ x3, const float* __restrict__ h3,
                                                       const float* __restrict__ hprev, float* __restrict__ hout, size_t items,
                                                       int Ch) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= items) return;
    const int L = Ch >> 2;
    const size_t m = i / L;
    const int c = (int)(i - m * L) * 4;
    const size_t o3 = m * 3 * Ch + c, o1 = m * Ch + c;
    float xr[4], xz[4], xn[4], hr[4] = {0.f, 0.f, 0.f, 0.f}, hz[4] = {0.f, 0.f, 0.f, 0.f}, hn[4] = {0.f, 0.f, 0.f, 0.f},
                               hp[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
    un(ld4(x3 + o3), xr), un(ld4(x3 + o3 + Ch), xz), un(ld4(x3 + o3 + 2 * Ch), xn);
    if (h3) un(ld4(h3 + o3), hr), un(ld4(h3 + o3 + Ch), hz), un(ld4(h3 + o3 + 2 * Ch), hn), un(ld4(hprev + o1), hp);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const Gate g = gate(xr[e], xz[e], xn[e], hr[e], hz[e], hn[e]);
        out[e] = fmaf(g.z, hp[e] - g.n, g.n);  // (1 - z) n + z h
    }
    st(hout + o1, out);
}

__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* __restrict__ x3, const float* __restrict__ h3,
                                                       const float* __restrict__ hprev, const float* __restrict__ go,
                                                       float* __restrict__ gx3, float* __restrict__ gh3, float* __restrict__ ghp,
                                                       size_t items, int Ch) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= items) return;
    const int L = Ch >> 2;
    const size_t m = i / L;
    const int c = (int)(i - m * L) * 4;
    const size_t o3 = m * 3 * Ch + c, o1 = m * Ch + c;
    float xr[4], xz[4], xn[4], hr[4] = {0.f, 0.f, 0.f, 0.f}, hz[4] = {0.f, 0.f, 0.f, 0.f}, hn[4] = {0.f, 0.f, 0.f, 0.f},
                               hp[4] = {0.f, 0.f, 0.f, 0.f}, g[4];
    un(ld4(x3 + o3), xr), un(ld4(x3 + o3 + Ch), xz), un(ld4(x3 + o3 + 2 * Ch), xn), un(ld4(go + o1), g);
    if (h3) un(ld4(h3 + o3), hr), un(ld4(h3 + o3 + Ch), hz), un(ld4(h3 + o3 + 2 * Ch), hn), un(ld4(hprev + o1), hp);
    float dr[4], dz[4], dn[4], dhn[4], dhp[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const Gate t = gate(xr[e], xz[e], xn[e], hr[e], hz[e], hn[e]);
        const float da_n = g[e] * (1.f - t.z) * (1.f - t.n * t.n);
        dn[e] = da_n;
        dhn[e] = da_n * t.r;
        dr[e] = da_n * hn[e] * t.r * (1.f - t.r);
        dz[e] = g[e] * (hp[e] - t.n) * t.z * (1.f - t.z);
        dhp[e] = g[e] * t.z;
    }
    st(gx3 + o3, dr), st(gx3 + o3 + Ch, dz), st(gx3 + o3 + 2 * Ch, dn);
    if (gh3) st(gh3 + o3, dr), st(gh3 + o3 + Ch, dz), st(gh3 + o3 + 2 * Ch, dhn);
    if (ghp) st(ghp + o1, dhp);
}

}  // namespace

int cp_launch_gru_gate_forward(hipStream_t s, const float* x3, const float* h3, const float* hprev, float* hout, long long M, int Ch) {
    const size_t items = (size_t)M * (Ch / 4);
    hipLaunchKernelGGL(gate_fwd_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, x3, h3, hprev, hout, items, Ch);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_gru_gate_backward(hipStream_t s, const float* x3, const float* h3, const float* hprev, const float* go, float* gx3,
                                float* gh3, float* ghp, long long M, int Ch) {
    const size_t items = (size_t)M * (Ch / 4);
    hipLaunchKernelGGL(gate_bwd_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, x3, h3, hprev, go, gx3, gh3, ghp, items,
                       Ch);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
