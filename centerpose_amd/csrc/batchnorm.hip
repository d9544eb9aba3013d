// BatchNorm2d for training, fused with the residual add and the ReLU (cp_batchnorm_forward_nhwc / cp_batchnorm_backward_nhwc):
// y = act((x - mean) * invstd * gamma + beta [+ residual]) on float32 NHWC tensors with the batch's own statistics (training)
// or the running ones (evaluation), and autograd's gradients of it.  It replaces the nn.BatchNorm2d -> `out += residual` ->
// ReLU chains of pose_dla_dcn.py:40-62 (BasicBlock), pose_dla_dcn.py:150-168 (Root), pose_dla_dcn.py:381 (the DCN's actf) and
// resnet_dcn.py.  Float32 arithmetic, no atomics, every sum in a fixed order that depends on the shape alone.
//
// All five streaming kernels share one thread map (lane_of, norm_common.h); groupnorm.hip uses the same map and the same
// per-slab statistics.
//
// On the caller's stream:
//   forward, training    stats_kernel     per slab and channel: mean and M2 = sum (x - mean)^2.  A lane sums d = x - pivot and d^2
//                                         about its own first row (E[x^2] - mean^2 from raw sums loses every digit at
//                                         |mean| >> std); lanes are merged by Chan's rule in its many-way form: mean = ref +
//                                         sum n_i (m_i - ref) / n, M2 = sum M2_i + n_i (m_i - mean)^2, in lane order.
//                        finalize_kernel  the slabs merged by the same rule, each round a two_level_sum (op_common.h); writes
//                                         save_mean, save_invstd, updates the running pair.
//   forward, evaluation  eval_stats_kernel  save_mean / save_invstd from the running pair.
//   forward              apply_kernel     y, whole lines in and out.
//   backward             bwd_reduce_kernel / bwd_finalize_kernel   grad_beta = sum g, grad_gamma = sum g * xhat (g gated by y > 0)
//                        bwd_apply_kernel grad_x (and grad_residual = g when asked) in one pass.
//
// SyncBatchNorm (cp_batchnorm_sync_*): the same kernels in phases around the caller's two all-gathers.  A rank is one more
// level of the Chan merge (chan_merge, shared by all three merging kernels):
//   forward A   stats_kernel, sync_record_kernel    this rank's record mean[C] | M2[C] | count
//   forward B   sync_merge_kernel, apply_kernel     the ranks' records merged in rank order; the global count stays on the device
//   backward A  bwd_reduce_kernel, bwd_finalize_kernel   this rank's two sums against the global mean
//   backward B  sync_sum_kernel, bwd_apply_kernel   the ranks' sums added in rank order; n read from the device
#include "norm_common.h"

#include <algorithm>

namespace {

// part[slab][0][c] = the slab's mean, part[slab][1][c] = its M2
__global__ __launch_bounds__(256) void stats_kernel(const float* __restrict__ x, float* __restrict__ part, int P, int C, int slab_px) {
    __shared__ float4 sm[256], sq[256];
    const Lane ln = lane_of(C);
    const int q_beg = blockIdx.x * slab_px, len = min(P - q_beg, slab_px);
    slab_stats(x + (size_t)q_beg * C, len, C, ln, part + (size_t)blockIdx.x * 2 * C, sm, sq);
}

// Chan's many-way merge of `nparts` partial statistics of one channel, in two rounds of two_level_sum: the mean about part 0's,
// then M2 about that mean.  rows(s), mean_of(s), m2_of(s): part s's count (as a float), mean and M2; n: the total count.  The
// slabs of a tensor (finalize_kernel, sync_record_kernel) and the ranks of a process group (sync_merge_kernel) are merged by
// these expressions and no others, so a merge of one part about its own mean adds exact zeros.  Every thread of the workgroup
// must call it (two barriers).
template <class N, class M, class Q>
__device__ __forceinline__ void chan_merge(float (&red)[256], bool cv, int nparts, float n, N rows, M mean_of, Q m2_of, float& mean,
                                           float& M2) {
    const float ref = cv ? mean_of(0) : 0.f;
    const float t = two_level_sum(red, cv, nparts, 0.f, [&](float a, int s) { return fmaf(rows(s), mean_of(s) - ref, a); });
    mean = ref + t / n;
    __syncthreads();
    M2 = two_level_sum(red, cv, nparts, 0.f, [&](float b, int s) {
        const float d = mean_of(s) - mean;
        return b + fmaf(rows(s) * d, d, m2_of(s));
    });
}
// the slabs of stats_kernel's part[slab][2][C], channel c
__device__ __forceinline__ void slab_merge(float (&red)[256], bool cv, const float* __restrict__ part, int c, int P, int C, int slab_px,
                                           int nslab, float& mean, float& M2) {
    chan_merge(
        red, cv, nslab, (float)P, [&](int s) { return (float)min(slab_px, P - s * slab_px); },
        [&](int s) { return part[(size_t)s * 2 * C + c]; }, [&](int s) { return part[(size_t)s * 2 * C + C + c]; }, mean, M2);
}
// what the forward keeps of a channel's merged statistics over n values
__device__ __forceinline__ void store_stats(int c, float mean, float M2, float n, float* __restrict__ save_mean,
                                            float* __restrict__ save_invstd, float* __restrict__ rmean, float* __restrict__ rvar,
                                            float momentum, float eps) {
    save_mean[c] = mean;
    save_invstd[c] = 1.f / sqrtf(M2 / n + eps);
    if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean;
    if (rvar) rvar[c] = (1.f - momentum) * rvar[c] + momentum * (M2 / (n - 1.f));
}

// The slabs merged per channel, 32 channels per workgroup.
__global__ __launch_bounds__(256) void finalize_kernel(const float* __restrict__ part, float* __restrict__ save_mean,
                                                       float* __restrict__ save_invstd, float* __restrict__ rmean,
                                                       float* __restrict__ rvar, int P, int C, int slab_px, int nslab, float momentum,
                                                       float eps) {
    __shared__ float red[256];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31);
    const bool cv = c < C;
    float mean, M2;
    slab_merge(red, cv, part, c, P, C, slab_px, nslab, mean, M2);
    if (threadIdx.x >= 32 || !cv) return;
    store_stats(c, mean, M2, (float)P, save_mean, save_invstd, rmean, rvar, momentum, eps);
}

// ---- SyncBatchNorm: the same statistics with one more level of the merge, the ranks of a process group ----
// A rank's record is mean[C] | M2[C] | count: the count of values per channel as a 32-bit integer's bit pattern in the first
// word of the last 16-byte slot (a float would round it above 2^24; an all-gather moves bits unchanged), the slot's other
// three words zero.
constexpr int kCountSlot = 4;

// forward, phase A: this rank's slabs merged exactly as finalize_kernel merges them -> its record
__global__ __launch_bounds__(256) void sync_record_kernel(const float* __restrict__ part, float* __restrict__ record, int P, int C,
                                                          int slab_px, int nslab) {
    __shared__ float red[256];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31);
    const bool cv = c < C;
    float mean, M2;
    slab_merge(red, cv, part, c, P, C, slab_px, nslab, mean, M2);
    if (blockIdx.x == 0 && threadIdx.x == 0) *reinterpret_cast<int4*>(record + 2 * C) = make_int4(P, 0, 0, 0);
    if (threadIdx.x >= 32 || !cv) return;
    record[c] = mean;
    record[C + c] = M2;
}

// forward, phase B: records[world][2C + 4] merged in rank order about rank 0's mean; every rank computes the same bits.  The
// global count goes to *save_count as a float, (float)P's rounding of it: what the backward divides by.
__global__ __launch_bounds__(256) void sync_merge_kernel(const float* __restrict__ records, int world, float* __restrict__ save_mean,
                                                         float* __restrict__ save_invstd, float* __restrict__ rmean,
                                                         float* __restrict__ rvar, float* __restrict__ save_count, int C,
                                                         float momentum, float eps) {
    __shared__ float red[256];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31);
    const bool cv = c < C;
    const size_t rec = (size_t)2 * C + kCountSlot;
    auto count = [&](int r) { return *reinterpret_cast<const int*>(records + r * rec + 2 * C); };
    unsigned long long total = 0;
    for (int r = 0; r < world; ++r) total += (unsigned)count(r);
    const float n = (float)total;
    float mean, M2;
    chan_merge(
        red, cv, world, n, [&](int r) { return (float)count(r); }, [&](int r) { return records[r * rec + c]; },
        [&](int r) { return records[r * rec + C + c]; }, mean, M2);
    if (blockIdx.x == 0 && threadIdx.x == 0) *save_count = n;
    if (threadIdx.x >= 32 || !cv) return;
    store_stats(c, mean, M2, n, save_mean, save_invstd, rmean, rvar, momentum, eps);
}

// backward, phase B: sums[i] = sums_all[0][i] + sums_all[1][i] + ..., ranks ascending (a backend's SUM has an order of its own)
__global__ __launch_bounds__(256) void sync_sum_kernel(const float* __restrict__ sums_all, float* __restrict__ sums, int world,
                                                       int C2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < C2) sums[i] = serial_sum(sums_all + C2, world - 1, (size_t)C2, (size_t)i, sums_all[i]);
}

__global__ void eval_stats_kernel(const float* __restrict__ rmean, const float* __restrict__ rvar, float* __restrict__ save_mean,
                                  float* __restrict__ save_invstd, int C, float eps) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    save_mean[c] = rmean[c];
    save_invstd[c] = 1.f / sqrtf(rvar[c] + eps);
}

// y = act((x - mean) * (invstd * gamma) + beta [+ res])
__global__ __launch_bounds__(256) void apply_kernel(const float* __restrict__ x, const float* __restrict__ res, float* __restrict__ y,
                                                    const float* __restrict__ mean, const float* __restrict__ invstd,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, int P, int C,
                                                    int slab_px, int act) {
    const Lane ln = lane_of(C);
    const int q_beg = blockIdx.x * slab_px, len = min(P - q_beg, slab_px);
    const int n = ln.active ? rows_of(len, ln.k, ln.S) : 0;
    if (n == 0) return;
    float mu[4], a[4], sh[4] = {0.f, 0.f, 0.f, 0.f};
    un4(ld4(mean + ln.c), mu);
    un4(ld4(invstd + ln.c), a);
    if (gamma) {
        float g[4];
        un4(ld4(gamma + ln.c), g);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] *= g[i];
    }
    if (beta) un4(ld4(beta + ln.c), sh);
    size_t off = (size_t)(q_beg + ln.k) * C + ln.c;
    const size_t step = (size_t)ln.S * C;
    auto put = [&](size_t o, const float4 v4, const float4 r4) {
        float v[4], r[4], out[4];
        un4(v4, v);
        un4(r4, r);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = fmaf(v[i] - mu[i], a[i], sh[i]) + r[i];
            out[i] = act ? cp_relu(t) : t;
        }
        st4(y + o, out);
    };
    auto ldr = [&](size_t o) { return res ? ld4(res + o) : zero4(); };
    int j = 0;
    for (; j + 4 <= n; j += 4, off += 4 * step) {
        const float4 v0 = ld4(x + off), v1 = ld4(x + off + step), v2 = ld4(x + off + 2 * step), v3 = ld4(x + off + 3 * step);
        const float4 r0 = ldr(off), r1 = ldr(off + step), r2 = ldr(off + 2 * step), r3 = ldr(off + 3 * step);
        put(off, v0, r0), put(off + step, v1, r1), put(off + 2 * step, v2, r2), put(off + 3 * step, v3, r3);
    }
    for (; j < n; ++j, off += step) put(off, ld4(x + off), ldr(off));
}

// part[slab][0][c] = sum g, part[slab][1][c] = sum g * (x - mean) over the slab's rows: rows ascending per lane, then the row
// phases in order
__global__ __launch_bounds__(256) void bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ go, const float* __restrict__ mean,
                                                         float* __restrict__ part, int P, int C, int slab_px) {
    __shared__ float4 sg[256], sx[256];
    const Lane ln = lane_of(C);
    const int q_beg = blockIdx.x * slab_px, len = min(P - q_beg, slab_px);
    const int n = ln.active ? rows_of(len, ln.k, ln.S) : 0;
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    if (n > 0) {
        float mu[4];
        un4(ld4(mean + ln.c), mu);
        size_t off = (size_t)(q_beg + ln.k) * C + ln.c;
        const size_t step = (size_t)ln.S * C;
        auto ldg = [&](size_t o) {
            const float4 g = ld4(go + o);
            return y ? gate4(g, ld4(y + o)) : g;
        };
        auto add = [&](const float4 g4, const float4 v4) {
            float g[4], v[4];
            un4(g4, g);
            un4(v4, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s1[i] += g[i];
                s2[i] = fmaf(g[i], v[i] - mu[i], s2[i]);
            }
        };
        int j = 0;
        for (; j + 2 <= n; j += 2, off += 2 * step) {
            const float4 v0 = ld4(x + off), v1 = ld4(x + off + step);
            const float4 g0 = ldg(off), g1 = ldg(off + step);
            add(g0, v0), add(g1, v1);
        }
        for (; j < n; ++j, off += step) add(ldg(off), ld4(x + off));
    }
    if (!slab_sum2(s1, s2, ln, sg, sx)) return;
    float* out = part + (size_t)blockIdx.x * 2 * C + ln.c;
    st4(out, s1);
    st4(out + C, s2);
}

// sums[0][c] = grad_beta, sums[1][c] = grad_gamma = invstd * sum g (x - mean), both by one two_level_sum over the slabs; the
// caller's grad_beta / grad_gamma get a copy when given
__global__ __launch_bounds__(256) void bwd_finalize_kernel(const float* __restrict__ part, const float* __restrict__ invstd,
                                                           float* __restrict__ sums, float* __restrict__ gg, float* __restrict__ gb,
                                                           int C, int nslab) {
    __shared__ Sum2 red[256];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31);
    const bool cv = c < C;
    Sum2 t = two_level_sum(red, cv, nslab, Sum2{0.f, 0.f}, [&](Sum2 v, int s) {
        const float* ps = part + (size_t)s * 2 * C + c;
        return v + Sum2{ps[0], ps[C]};
    });
    if (threadIdx.x >= 32 || !cv) return;
    t.b *= invstd[c];
    sums[c] = t.a;
    sums[C + c] = t.b;
    if (gb) gb[c] = t.a;
    if (gg) gg[c] = t.b;
}

// training: grad_x = gamma * invstd * (g - grad_beta / n - xhat * grad_gamma / n); evaluation: gamma * invstd * g;
// grad_residual = g.  gx or gres may be null (not both).  n is P, or *count where given (the sync backward: the global count
// the forward left on the device, with `sums` the global sums).
__global__ __launch_bounds__(256) void bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ go, const float* __restrict__ gamma,
                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        const float* __restrict__ sums, float* __restrict__ gx,
                                                        float* __restrict__ gres, int P, int C, int slab_px, int training,
                                                        const float* __restrict__ count) {
    const Lane ln = lane_of(C);
    const int q_beg = blockIdx.x * slab_px, len = min(P - q_beg, slab_px);
    const int n = ln.active ? rows_of(len, ln.k, ln.S) : 0;
    if (n == 0) return;
    const bool need_x = training && gx;  // (x enters grad_x only through the batch statistics)
    float mu[4] = {0.f, 0.f, 0.f, 0.f}, a[4], k1[4] = {0.f, 0.f, 0.f, 0.f}, k2[4] = {0.f, 0.f, 0.f, 0.f};
    un4(ld4(invstd + ln.c), a);
    if (need_x) {
        float s1[4], s2[4];
        const float rn = 1.f / (count ? *count : (float)P);
        un4(ld4(mean + ln.c), mu);
        un4(ld4(sums + ln.c), s1);
        un4(ld4(sums + C + ln.c), s2);
#pragma unroll
        for (int i = 0; i < 4; ++i) k1[i] = s1[i] * rn, k2[i] = s2[i] * rn * a[i];
    }
    if (gamma) {
        float g[4];
        un4(ld4(gamma + ln.c), g);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] *= g[i];
    }
    size_t off = (size_t)(q_beg + ln.k) * C + ln.c;
    const size_t step = (size_t)ln.S * C;
    auto ldg = [&](size_t o) {
        const float4 g = ld4(go + o);
        return y ? gate4(g, ld4(y + o)) : g;
    };
    auto ldx = [&](size_t o) { return need_x ? ld4(x + o) : zero4(); };
    auto put = [&](size_t o, const float4 g4, const float4 v4) {
        float g[4], v[4], out[4];
        un4(g4, g);
        un4(v4, v);
        if (gres) st4(gres + o, g);
        if (!gx) return;
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = a[i] * (g[i] - k1[i] - (v[i] - mu[i]) * k2[i]);
        st4(gx + o, out);
    };
    int j = 0;
    for (; j + 2 <= n; j += 2, off += 2 * step) {
        const float4 g0 = ldg(off), g1 = ldg(off + step);
        const float4 v0 = ldx(off), v1 = ldx(off + step);
        put(off, g0, v0), put(off + step, g1, v1);
    }
    for (; j < n; ++j, off += step) put(off, ldg(off), ldx(off));
}

// Slabs of whole workgroup steps (S rows).  Reductions: at least eight steps per slab and at most about 2048 workgroups, so the
// partials stay small and the finalize short; element-wise passes: eight steps per workgroup.
struct Plan {
    int P, npass, S;
    int red_px, red_slabs, red_bound;  // rows per slab, slabs, and a bound on them that is monotone in P (sizes the workspace)
    int app_px, app_slabs;
};

Plan plan(int B, int H, int W, int C) {
    Plan p;
    const int L = C / 4, CL = std::min(L, 64);
    p.P = B * H * W;
    p.npass = (L + 63) / 64;
    p.S = 4 * (64 / CL);
    const int steps = (p.P + p.S - 1) / p.S;
    p.red_bound = std::max(1, std::min((steps + 7) / 8, std::max(1, 2048 / p.npass)));
    p.red_px = (steps + p.red_bound - 1) / p.red_bound * p.S;
    p.red_slabs = (p.P + p.red_px - 1) / p.red_px;
    p.app_px = 8 * p.S;
    p.app_slabs = (p.P + p.app_px - 1) / p.app_px;
    return p;
}

struct Ws {
    float *part, *sums;  // the slabs' partials [slab][2][C]; the backward's two sums [2][C]
};
Ws bn_carve(Carve& c, const Plan& p, int C) {
    Ws r;
    r.part = c.take<float>((size_t)p.red_bound * 2 * C * 4);
    r.sums = c.take<float>((size_t)2 * C * 4);
    return r;
}

}  // namespace

size_t cp_batchnorm_ws_bytes(int B, int H, int W, int C) {
    Carve c{nullptr};
    bn_carve(c, plan(B, H, W, C), C);
    return c.off;
}

int cp_launch_batchnorm_forward(hipStream_t s, const BnFwdArgs& a, void* ws) {
    const Plan p = plan(a.B, a.H, a.W, a.C);
    Carve cv{(char*)ws};
    float* part = bn_carve(cv, p, a.C).part;
    if (a.training) {
        hipLaunchKernelGGL(stats_kernel, dim3(p.red_slabs, p.npass), dim3(256), 0, s, a.x, part, p.P, a.C, p.red_px);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        hipLaunchKernelGGL(finalize_kernel, dim3((a.C + 31) / 32), dim3(256), 0, s, (const float*)part, a.mean, a.invstd, a.rmean,
                           a.rvar, p.P, a.C, p.red_px, p.red_slabs, a.momentum, a.eps);
    } else {
        hipLaunchKernelGGL(eval_stats_kernel, dim3((a.C + 255) / 256), dim3(256), 0, s, (const float*)a.rmean, (const float*)a.rvar,
                           a.mean, a.invstd, a.C, a.eps);
    }
    if (!launch_ok()) return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(apply_kernel, dim3(p.app_slabs, p.npass), dim3(256), 0, s, a.x, a.res, a.y, (const float*)a.mean,
                       (const float*)a.invstd, a.gamma, a.beta, p.P, a.C, p.app_px, a.act);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_batchnorm_backward(hipStream_t s, const BnBwdArgs& a, void* ws) {
    const Plan p = plan(a.B, a.H, a.W, a.C);
    Carve cv{(char*)ws};
    const Ws r = bn_carve(cv, p, a.C);
    float *part = r.part, *sums = r.sums;
    if (a.gg || a.gb || (a.training && a.gx)) {
        hipLaunchKernelGGL(bwd_reduce_kernel, dim3(p.red_slabs, p.npass), dim3(256), 0, s, a.x, a.y, a.go, a.mean, part, p.P, a.C,
                           p.red_px);
        if (!launch_ok()) return CP_ERR_LAUNCH;
        hipLaunchKernelGGL(bwd_finalize_kernel, dim3((a.C + 31) / 32), dim3(256), 0, s, (const float*)part, a.invstd, sums, a.gg,
                           a.gb, a.C, p.red_slabs);
        if (!launch_ok()) return CP_ERR_LAUNCH;
    }
    if (!a.gx && !a.gres) return CP_OK;
    hipLaunchKernelGGL(bwd_apply_kernel, dim3(p.app_slabs, p.npass), dim3(256), 0, s, a.x, a.y, a.go, a.gamma, a.mean, a.invstd,
                       (const float*)sums, a.gx, a.gres, p.P, a.C, p.app_px, a.training, (const float*)nullptr);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_batchnorm_sync_rec_floats(int C) { return 2 * C + kCountSlot; }

int cp_launch_batchnorm_sync_stats(hipStream_t s, const float* x, float* record, int B, int H, int W, int C, void* ws) {
    const Plan p = plan(B, H, W, C);
    Carve cv{(char*)ws};
    float* part = bn_carve(cv, p, C).part;
    hipLaunchKernelGGL(stats_kernel, dim3(p.red_slabs, p.npass), dim3(256), 0, s, x, part, p.P, C, p.red_px);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(sync_record_kernel, dim3((C + 31) / 32), dim3(256), 0, s, (const float*)part, record, p.P, C, p.red_px,
                       p.red_slabs);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_batchnorm_sync_forward(hipStream_t s, const BnFwdArgs& a, const float* records, int world, float* save_count) {
    const Plan p = plan(a.B, a.H, a.W, a.C);
    hipLaunchKernelGGL(sync_merge_kernel, dim3((a.C + 31) / 32), dim3(256), 0, s, records, world, a.mean, a.invstd, a.rmean, a.rvar,
                       save_count, a.C, a.momentum, a.eps);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(apply_kernel, dim3(p.app_slabs, p.npass), dim3(256), 0, s, a.x, a.res, a.y, (const float*)a.mean,
                       (const float*)a.invstd, a.gamma, a.beta, p.P, a.C, p.app_px, a.act);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

// a.mean / a.invstd: the global pair; sums [2][C], a.gg, a.gb: this rank's own sums
int cp_launch_batchnorm_sync_backward_reduce(hipStream_t s, const BnBwdArgs& a, float* sums, void* ws) {
    const Plan p = plan(a.B, a.H, a.W, a.C);
    Carve cv{(char*)ws};
    float* part = bn_carve(cv, p, a.C).part;
    hipLaunchKernelGGL(bwd_reduce_kernel, dim3(p.red_slabs, p.npass), dim3(256), 0, s, a.x, a.y, a.go, a.mean, part, p.P, a.C,
                       p.red_px);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(bwd_finalize_kernel, dim3((a.C + 31) / 32), dim3(256), 0, s, (const float*)part, a.invstd, sums, a.gg, a.gb,
                       a.C, p.red_slabs);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_batchnorm_sync_backward_apply(hipStream_t s, const BnBwdArgs& a, const float* sums_all, int world,
                                            const float* save_count, void* ws) {
    const Plan p = plan(a.B, a.H, a.W, a.C);
    Carve cv{(char*)ws};
    float* sums = bn_carve(cv, p, a.C).sums;
    if (a.gx) {
        hipLaunchKernelGGL(sync_sum_kernel, dim3((2 * a.C + 255) / 256), dim3(256), 0, s, sums_all, sums, world, 2 * a.C);
        if (!launch_ok()) return CP_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(bwd_apply_kernel, dim3(p.app_slabs, p.npass), dim3(256), 0, s, a.x, a.y, a.go, a.gamma, a.mean, a.invstd,
                       (const float*)sums, a.gx, a.gres, p.P, a.C, p.app_px, 1, save_count);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
