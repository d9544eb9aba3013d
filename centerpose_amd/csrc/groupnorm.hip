// GroupNorm for training, fused with the ReLU (cp_groupnorm_forward_nhwc / cp_groupnorm_backward_nhwc): nn.GroupNorm(G, C) on
// float32 NHWC tensors, y = act(xhat * gamma + beta), and autograd's gradients of it.  It is the normalisation of the dlav1_34
// heads (pose_dla_dcn.py:491-521 with GN.py's group rule).  Float32 arithmetic, no atomics, every sum in a fixed order that
// depends on the shape alone.
//
// The statistics are per (image, group) over n = (C / G) H W values.  The streaming kernels use batchnorm.hip's thread map
// (lane_of, norm_common.h) on the P = H W rows of ONE image: a slab never straddles two images, blockIdx.x = image * slabs +
// slab, blockIdx.y = channel pass.  A lane's float4 lies inside one group (C / G a multiple of 4) or holds whole groups
// (C / G = 1 or 2), so a lane reads at most four (mean, invstd) pairs.
//
// On the caller's stream:
//   forward   stats_kernel      per (image, slab, channel): mean and M2, exactly batchnorm.hip's (slab_stats).
//             finalize_kernel   per (image, group): the slabs x channels of the group merged by Chan's rule, each round a
//                               two_level_sum over the items j = slab * (C / G) + channel; writes save_mean, save_invstd.
//             apply_kernel      y, whole lines in and out.
//   backward  bwd_reduce_kernel    per (image, slab, channel): sum g and sum g (x - mean), g gated by y > 0.
//             bwd_finalize_kernel  two kinds of workgroup in one launch: per (image, group) s1 = sum g gamma and s2 = sum g
//                                  gamma xhat over the group's slabs x channels; per channel grad_beta = sum g and grad_gamma
//                                  = sum g xhat over images x slabs (images ascending within each of two_level_sum's lanes).
//             bwd_apply_kernel     grad_x = invstd (g gamma - s1 / n - xhat s2 / n) in one pass.
#include "norm_common.h"

#include <algorithm>

namespace {

// the per-image geometry every kernel gets
struct Geo {
    int P, C, G, cpg;  // rows per image, channels, groups, channels per group
    int slab_px, nslab;
};

// this workgroup's image, and its slab's first row and length
struct Slab {
    int img, q_beg, len;
};
__device__ __forceinline__ Slab slab_of(const Geo& g) {
    Slab s;
    s.img = blockIdx.x / g.nslab;
    s.q_beg = (blockIdx.x - s.img * g.nslab) * g.slab_px;
    s.len = min(g.P - s.q_beg, g.slab_px);
    return s;
}

// the (image, group) values of a lane's four channels
__device__ __forceinline__ void ld_group4(const float* __restrict__ v, const Geo& g, int img, int c, float (&o)[4]) {
    const float* p = v + (size_t)img * g.G;
    if (g.cpg >= 4) {
        o[0] = o[1] = o[2] = o[3] = p[c / g.cpg];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = p[(c + i) / g.cpg];
    }
}

// part[image * nslab + slab][0][c] = the slab's mean, [1][c] = its M2
__global__ __launch_bounds__(256) void stats_kernel(const float* __restrict__ x, float* __restrict__ part, Geo g) {
    __shared__ float4 sm[256], sq[256];
    const Lane ln = lane_of(g.C);
    const Slab s = slab_of(g);
    slab_stats(x + ((size_t)s.img * g.P + s.q_beg) * g.C, s.len, g.C, ln, part + (size_t)blockIdx.x * 2 * g.C, sm, sq);
}

// 32 groups of one image per workgroup (blockIdx.x = image * nb + block of groups).  The items of a group are its (slab,
// channel) partials, j = slab * cpg + channel, each over rows(slab) values: the mean about item 0's, then M2 about that mean.
__global__ __launch_bounds__(256) void finalize_kernel(const float* __restrict__ part, float* __restrict__ save_mean,
                                                       float* __restrict__ save_invstd, Geo g, int nb, float eps) {
    __shared__ float red[256];
    const int img = blockIdx.x / nb, grp = (blockIdx.x - img * nb) * 32 + (threadIdx.x & 31);
    const bool gv = grp < g.G;
    const float* pi = part + (size_t)img * g.nslab * 2 * g.C + (gv ? grp * g.cpg : 0);
    const int items = g.nslab * g.cpg;
    const float ref = gv ? pi[0] : 0.f, n = (float)g.cpg * (float)g.P;
    auto rows = [&](int s) { return (float)min(g.slab_px, g.P - s * g.slab_px); };
    const float t = two_level_sum(red, gv, items, 0.f, [&](float a, int j) {
        const int s = j / g.cpg, ci = j - s * g.cpg;
        return fmaf(rows(s), pi[(size_t)s * 2 * g.C + ci] - ref, a);
    });
    const float mean = ref + t / n;
    __syncthreads();
    const float M2 = two_level_sum(red, gv, items, 0.f, [&](float b, int j) {
        const int s = j / g.cpg, ci = j - s * g.cpg;
        const float* ps = pi + (size_t)s * 2 * g.C + ci;
        const float d = ps[0] - mean;
        return b + fmaf(rows(s) * d, d, ps[g.C]);
    });
    if (threadIdx.x >= 32 || !gv) return;
    save_mean[(size_t)img * g.G + grp] = mean;
    save_invstd[(size_t)img * g.G + grp] = 1.f / sqrtf(M2 / n + eps);
}

// y = act((x - mean) * (invstd * gamma) + beta)
__global__ __launch_bounds__(256) void apply_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ mean,
                                                    const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, Geo g, int act) {
    const Lane ln = lane_of(g.C);
    const Slab s = slab_of(g);
    const int n = ln.active ? rows_of(s.len, ln.k, ln.S) : 0;
    if (n == 0) return;
    float mu[4], a[4], sh[4] = {0.f, 0.f, 0.f, 0.f};
    ld_group4(mean, g, s.img, ln.c, mu);
    ld_group4(invstd, g, s.img, ln.c, a);
    if (gamma) {
        float w[4];
        un4(ld4(gamma + ln.c), w);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] *= w[i];
    }
    if (beta) un4(ld4(beta + ln.c), sh);
    size_t off = ((size_t)s.img * g.P + s.q_beg + ln.k) * g.C + ln.c;
    const size_t step = (size_t)ln.S * g.C;
    auto put = [&](size_t o, const float4 v4) {
        float v[4], out[4];
        un4(v4, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = fmaf(v[i] - mu[i], a[i], sh[i]);
            out[i] = act ? cp_relu(t) : t;
        }
        st4(y + o, out);
    };
    int j = 0;
    for (; j + 4 <= n; j += 4, off += 4 * step) {
        const float4 v0 = ld4(x + off), v1 = ld4(x + off + step), v2 = ld4(x + off + 2 * step), v3 = ld4(x + off + 3 * step);
        put(off, v0), put(off + step, v1), put(off + 2 * step, v2), put(off + 3 * step, v3);
    }
    for (; j < n; ++j, off += step) put(off, ld4(x + off));
}

// part[image * nslab + slab][0][c] = sum g, [1][c] = sum g * (x - mean) over the slab's rows: rows ascending per lane, then the
// row phases in order
__global__ __launch_bounds__(256) void bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ go, const float* __restrict__ mean,
                                                         float* __restrict__ part, Geo g) {
    __shared__ float4 sg[256], sx[256];
    const Lane ln = lane_of(g.C);
    const Slab s = slab_of(g);
    const int n = ln.active ? rows_of(s.len, ln.k, ln.S) : 0;
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    if (n > 0) {
        float mu[4];
        ld_group4(mean, g, s.img, ln.c, mu);
        size_t off = ((size_t)s.img * g.P + s.q_beg + ln.k) * g.C + ln.c;
        const size_t step = (size_t)ln.S * g.C;
        auto ldg = [&](size_t o) {
            const float4 t = ld4(go + o);
            return y ? gate4(t, ld4(y + o)) : t;
        };
        auto add = [&](const float4 g4, const float4 v4) {
            float t[4], v[4];
            un4(g4, t);
            un4(v4, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s1[i] += t[i];
                s2[i] = fmaf(t[i], v[i] - mu[i], s2[i]);
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
    float* out = part + (size_t)blockIdx.x * 2 * g.C + ln.c;
    st4(out, s1);
    st4(out + g.C, s2);
}

// Workgroups 0 .. ngb-1 (only when gs is given): 32 (image, group) pairs each, gs[image][group] = {s1, s2} over the group's items
// j = slab * cpg + channel.  Workgroups ngb ..: 32 channels each, grad_beta / grad_gamma over the items j = image * nslab + slab.
__global__ __launch_bounds__(256) void bwd_finalize_kernel(const float* __restrict__ part, const float* __restrict__ gamma,
                                                           const float* __restrict__ invstd, float* __restrict__ gs,
                                                           float* __restrict__ gg, float* __restrict__ gb, Geo g, int B, int ngb) {
    __shared__ Sum2 red[256];
    const int el = threadIdx.x & 31;
    if ((int)blockIdx.x < ngb) {
        const int e = blockIdx.x * 32 + el;
        const bool ev = e < B * g.G;
        const int img = ev ? e / g.G : 0, grp = ev ? e - img * g.G : 0;
        const float* pi = part + (size_t)img * g.nslab * 2 * g.C + grp * g.cpg;
        const float* w = gamma ? gamma + grp * g.cpg : nullptr;
        Sum2 t = two_level_sum(red, ev, g.nslab * g.cpg, Sum2{0.f, 0.f}, [&](Sum2 v, int j) {
            const int s = j / g.cpg, ci = j - s * g.cpg;
            const float* ps = pi + (size_t)s * 2 * g.C + ci;
            const float wc = w ? w[ci] : 1.f;
            return Sum2{fmaf(wc, ps[0], v.a), fmaf(wc, ps[g.C], v.b)};
        });
        if (threadIdx.x >= 32 || !ev) return;
        gs[2 * (size_t)e] = t.a;
        gs[2 * (size_t)e + 1] = t.b * invstd[e];
        return;
    }
    const int c = (blockIdx.x - ngb) * 32 + el;
    const bool cv = c < g.C;
    const int grp = cv ? c / g.cpg : 0;
    Sum2 t = two_level_sum(red, cv, B * g.nslab, Sum2{0.f, 0.f}, [&](Sum2 v, int j) {
        const float* ps = part + (size_t)j * 2 * g.C + c;
        return Sum2{v.a + ps[0], fmaf(invstd[(size_t)(j / g.nslab) * g.G + grp], ps[g.C], v.b)};
    });
    if (threadIdx.x >= 32 || !cv) return;
    if (gb) gb[c] = t.a;
    if (gg) gg[c] = t.b;
}

// grad_x = invstd * (g * gamma - s1 / n - xhat * s2 / n)
__global__ __launch_bounds__(256) void bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ go, const float* __restrict__ gamma,
                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        const float* __restrict__ gs, float* __restrict__ gx, Geo g) {
    const Lane ln = lane_of(g.C);
    const Slab s = slab_of(g);
    const int n = ln.active ? rows_of(s.len, ln.k, ln.S) : 0;
    if (n == 0) return;
    float mu[4], a[4], k1[4], k2[4];
    ld_group4(mean, g, s.img, ln.c, mu);
    ld_group4(invstd, g, s.img, ln.c, a);
    const float rn = 1.f / ((float)g.cpg * (float)g.P);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float* p = gs + 2 * ((size_t)s.img * g.G + (ln.c + i) / g.cpg);
        k1[i] = a[i] * p[0] * rn;
        k2[i] = a[i] * a[i] * p[1] * rn;
    }
    if (gamma) {
        float w[4];
        un4(ld4(gamma + ln.c), w);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] *= w[i];
    }
    size_t off = ((size_t)s.img * g.P + s.q_beg + ln.k) * g.C + ln.c;
    const size_t step = (size_t)ln.S * g.C;
    auto ldg = [&](size_t o) {
        const float4 t = ld4(go + o);
        return y ? gate4(t, ld4(y + o)) : t;
    };
    auto put = [&](size_t o, const float4 g4, const float4 v4) {
        float t[4], v[4], out[4];
        un4(g4, t);
        un4(v4, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = a[i] * t[i] - k1[i] - (v[i] - mu[i]) * k2[i];
        st4(gx + o, out);
    };
    int j = 0;
    for (; j + 2 <= n; j += 2, off += 2 * step) {
        const float4 g0 = ldg(off), g1 = ldg(off + step);
        const float4 v0 = ld4(x + off), v1 = ld4(x + off + step);
        put(off, g0, v0), put(off + step, g1, v1);
    }
    for (; j < n; ++j, off += step) put(off, ldg(off), ld4(x + off));
}

// Slabs of whole workgroup steps (S rows) of one image.  Reductions: at least eight steps per slab and at most kMaxSlabs per
// image (the images multiply the grid, and a group's finalize walks slabs x channels items); element-wise passes: eight steps
// per workgroup.
constexpr int kMaxSlabs = 128;
struct Plan {
    int npass;
    Geo red, app;
};

Plan plan(int H, int W, int C, int G) {
    Plan p;
    const int L = C / 4, CL = std::min(L, 64), S = 4 * (64 / CL), P = H * W;
    p.npass = (L + 63) / 64;
    const int steps = (P + S - 1) / S;
    const int bound = std::max(1, std::min((steps + 7) / 8, kMaxSlabs));
    p.red.P = p.app.P = P, p.red.C = p.app.C = C, p.red.G = p.app.G = G, p.red.cpg = p.app.cpg = C / G;
    p.red.slab_px = (steps + bound - 1) / bound * S;
    p.red.nslab = (P + p.red.slab_px - 1) / p.red.slab_px;
    p.app.slab_px = 8 * S;
    p.app.nslab = (P + p.app.slab_px - 1) / p.app.slab_px;
    return p;
}

struct Ws {
    float *part, *gs;  // the slabs' partials [image][slab][2][C]; the backward's group sums [image][group][2]
};
Ws gn_carve(Carve& c, const Plan& p, int B) {
    Ws r;
    r.part = c.take<float>((size_t)B * p.red.nslab * 2 * p.red.C * 4);
    r.gs = c.take<float>((size_t)B * p.red.G * 2 * 4);
    return r;
}

}  // namespace

size_t cp_groupnorm_ws_bytes(int B, int H, int W, int C, int G) {
    Carve c{nullptr};
    gn_carve(c, plan(H, W, C, G), B);
    return c.off;
}

int cp_launch_groupnorm_forward(hipStream_t s, const GnFwdArgs& a, void* ws) {
    const Plan p = plan(a.H, a.W, a.C, a.G);
    Carve cv{(char*)ws};
    float* part = gn_carve(cv, p, a.B).part;
    hipLaunchKernelGGL(stats_kernel, dim3(a.B * p.red.nslab, p.npass), dim3(256), 0, s, a.x, part, p.red);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    const int nb = (a.G + 31) / 32;
    hipLaunchKernelGGL(finalize_kernel, dim3(a.B * nb), dim3(256), 0, s, (const float*)part, a.mean, a.invstd, p.red, nb, a.eps);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(apply_kernel, dim3(a.B * p.app.nslab, p.npass), dim3(256), 0, s, a.x, a.y, (const float*)a.mean,
                       (const float*)a.invstd, a.gamma, a.beta, p.app, a.act);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_groupnorm_backward(hipStream_t s, const GnBwdArgs& a, void* ws) {
    if (!a.gx && !a.gg && !a.gb) return CP_OK;
    const Plan p = plan(a.H, a.W, a.C, a.G);
    Carve cv{(char*)ws};
    const Ws r = gn_carve(cv, p, a.B);
    hipLaunchKernelGGL(bwd_reduce_kernel, dim3(a.B * p.red.nslab, p.npass), dim3(256), 0, s, a.x, a.y, a.go, a.mean, r.part, p.red);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    const int ngb = a.gx ? (a.B * a.G + 31) / 32 : 0, ncb = a.gg || a.gb ? (a.C + 31) / 32 : 0;
    hipLaunchKernelGGL(bwd_finalize_kernel, dim3(ngb + ncb), dim3(256), 0, s, (const float*)r.part, a.gamma, a.invstd, r.gs, a.gg,
                       a.gb, p.red, a.B, ngb);
    if (!launch_ok()) return CP_ERR_LAUNCH;
    if (!a.gx) return CP_OK;
    hipLaunchKernelGGL(bwd_apply_kernel, dim3(a.B * p.app.nslab, p.npass), dim3(256), 0, s, a.x, a.y, a.go, a.gamma, a.mean, a.invstd,
                       (const float*)r.gs, a.gx, p.app);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
