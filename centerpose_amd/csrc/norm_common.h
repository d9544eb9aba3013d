// What the training normalisations share (batchnorm.hip, groupnorm.hip): the thread map of their streaming kernels and the
// per-slab statistics with Chan's merge.  The summation orders are contract (the tests compare bitwise), so they are written
// here once.
//
// The thread map (lane_of): a tensor is pixel rows of C floats; a wave reads 16 bytes per lane, so with L = C / 4 lanes per
// row, CL = min(L, 64) lanes take a row and a wave takes PW = 64 / CL rows at a time (C = 16: 16 rows, one 1 KiB run of whole
// 128-byte lines; C = 20: 12 rows, 60 of 64 lanes busy); rows wider than a wave (C > 256) are covered by ceil(L / 64) channel
// passes (blockIdx.y).  A workgroup is four waves on neighbouring rows and owns a slab of rows; a lane keeps its four channels
// for the whole slab, so the per-channel coefficients sit in registers and the sums need no shuffles.
#pragma once
#include "op_common.h"
#include "igemm_common.h"

struct Lane {
    bool active;  // this lane holds channels of this pass
    int c;        // its first channel
    int k, S;     // it owns the slab's rows k, k + S, ...
    int CL;       // lanes per row
};

__device__ __forceinline__ Lane lane_of(int C) {
    const int L = C >> 2, CL = min(L, 64), PW = 64 / CL;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pl = lane / CL, cl = lane - pl * CL, cg = blockIdx.y * 64 + cl;
    Lane ln;
    ln.active = pl < PW && cg < L;
    ln.c = 4 * cg;
    ln.k = w * PW + pl;
    ln.S = 4 * PW;
    ln.CL = CL;
    return ln;
}
// index into a 256-entry LDS table of the lane that owns row phase k of the same channels (k < S)
__device__ __forceinline__ int peer(const Lane& ln, int k) {
    const int PW = ln.S >> 2, w = k / PW, pl = k - w * PW;
    return w * 64 + pl * ln.CL + (threadIdx.x & 63) % ln.CL;
}
// rows of phase k in a slab of len rows
__device__ __forceinline__ int rows_of(int len, int k, int S) { return k < len ? (len - k + S - 1) / S : 0; }

__device__ __forceinline__ void st4(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void un4(const float4 v, float (&o)[4]) { o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w; }

__device__ __forceinline__ float4 gate4(const float4 g, const float4 y) {
    return make_float4(cp_relu_gate(g.x, y.x), cp_relu_gate(g.y, y.y), cp_relu_gate(g.z, y.z), cp_relu_gate(g.w, y.w));
}

// One slab's statistics per channel: out[0][c] = the mean, out[1][c] = M2 = sum (x - mean)^2 over the slab's `len` rows, which
// start at `rows`.  A lane sums d = x - pivot and d^2 about its own first row (E[x^2] - mean^2 from raw sums loses every digit
// at |mean| >> std); the row phases are merged by Chan's rule in its many-way form: mean = ref + sum n_i (m_i - ref) / n,
// M2 = sum M2_i + n_i (m_i - mean)^2, in phase order.  Every thread of the workgroup must call it (one barrier).
__device__ __forceinline__ void slab_stats(const float* __restrict__ rows, int len, int C, const Lane& ln, float* __restrict__ out,
                                           float4 (&sm)[256], float4 (&sq)[256]) {
    const int n = ln.active ? rows_of(len, ln.k, ln.S) : 0;
    float piv[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    if (n > 0) {
        const float* px = rows + (size_t)ln.k * C + ln.c;
        const size_t step = (size_t)ln.S * C;
        un4(ld4(px), piv);
        auto add = [&](const float4 v4) {
            float v[4];
            un4(v4, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float d = v[i] - piv[i];
                s1[i] += d;
                s2[i] = fmaf(d, d, s2[i]);
            }
        };
        int j = 0;
        for (; j + 4 <= n; j += 4) {  // four rows requested before the first is used
            const float4 v0 = ld4(px), v1 = ld4(px + step), v2 = ld4(px + 2 * step), v3 = ld4(px + 3 * step);
            px += 4 * step;
            add(v0), add(v1), add(v2), add(v3);
        }
        for (; j < n; ++j, px += step) add(ld4(px));
    }
    const float rn = n > 0 ? 1.f / (float)n : 0.f;
    float m[4], q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        m[i] = fmaf(s1[i], rn, piv[i]);
        q[i] = fmaxf(s2[i] - s1[i] * s1[i] * rn, 0.f);
    }
    sm[threadIdx.x] = make_float4(m[0], m[1], m[2], m[3]);
    sq[threadIdx.x] = make_float4(q[0], q[1], q[2], q[3]);
    __syncthreads();
    if (!ln.active || ln.k != 0) return;
    // the row phases in order; phase 0 (this lane) is never empty
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 1; k < ln.S; ++k) {
        const float nk = (float)rows_of(len, k, ln.S);
        float t[4];
        un4(sm[peer(ln, k)], t);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(nk, t[i] - m[i], acc[i]);
    }
    float mean[4], M2[4] = {0.f, 0.f, 0.f, 0.f};
    const float rl = 1.f / (float)len;
#pragma unroll
    for (int i = 0; i < 4; ++i) mean[i] = fmaf(acc[i], rl, m[i]);
    for (int k = 0; k < ln.S; ++k) {
        const float nk = (float)rows_of(len, k, ln.S);
        const int p = peer(ln, k);
        float t[4], u[4];
        un4(sm[p], t);
        un4(sq[p], u);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = t[i] - mean[i];
            M2[i] += fmaf(nk * d, d, u[i]);
        }
    }
    st4(out + ln.c, mean);
    st4(out + C + ln.c, M2);
}

// The row-phase merge of a slab's two running sums (the backward reductions): phase 0's lane adds the phases 1 .. S-1 in
// order.  Returns true on the lane that holds the result.  Every thread of the workgroup must call it (one barrier).
__device__ __forceinline__ bool slab_sum2(float (&s1)[4], float (&s2)[4], const Lane& ln, float4 (&sg)[256], float4 (&sx)[256]) {
    sg[threadIdx.x] = make_float4(s1[0], s1[1], s1[2], s1[3]);
    sx[threadIdx.x] = make_float4(s2[0], s2[1], s2[2], s2[3]);
    __syncthreads();
    if (!ln.active || ln.k != 0) return false;
    for (int k = 1; k < ln.S; ++k) {
        const int p = peer(ln, k);
        float t[4], u[4];
        un4(sg[p], t);
        un4(sx[p], u);
#pragma unroll
        for (int i = 0; i < 4; ++i) s1[i] += t[i], s2[i] += u[i];
    }
    return true;
}

struct Sum2 {
    float a, b;
};
__device__ __forceinline__ Sum2 operator+(const Sum2 x, const Sum2 y) { return {x.a + y.a, x.b + y.b}; }
