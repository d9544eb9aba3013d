// ObjectPoseLoss on the device (trains/object_pose.py:22-205): the focal heat-map terms, the gathered regression terms,
// the per-image choice of the symmetry variant, and the backward of the chosen variant.  Per-element formulas and their
// derivatives are in pose_loss_common.h.
//
//   1. focal_fwd_kernel   one pass over a heat-map head per stack: logit -> sigmoid (written back in place, _sigmoid's
//                         sigmoid_) and clamp(sigmoid) to `clamped`; per pixel log(p)(1-p)^2 and log(1-p)p^2 stay in
//                         registers while the S ground-truth slices stream past (pred is read once whatever S is).  Each
//                         workgroup writes (pos, neg, num_pos) per (b, s) to a partial slab; no atomics.
//   2. terms_kernel       one workgroup per (b, s, stack): sums the focal slabs in slab order (double) and finishes the
//                         focal loss with losses.py:69-74's num_pos == 0 branch; gathers and reduces every regression term.
//   3. select_kernel      one workgroup: per-variant weighted total summed over the stacks, valid = sum_k ind > 0,
//                         torch.argmin's choice, the mean of each chosen term over b, loss and the ten stats.
//   Backward:
//   4. focal_bwd_kernel   one pass over the chosen ground-truth slice and the in-place sigmoid -> dL/dlogit.
//   5. reg_bwd_kernel     one workgroup per (b, term, stack) after a zero-fill of the gradient heads: lane d owns channel d
//                         and walks the K gathered entries serially, so repeated indices add in a fixed order.
// Every sum has an order that depends on neither the run nor s: outputs are bitwise reproducible and identical variants
// give identical terms.
#include "../../include/centerpose_hip.h"
#include "cp_common.h"
#include "pose_loss_common.h"

#include <algorithm>

using namespace pose_loss;

namespace {

constexpr int FT = 256;                 // focal kernels: threads per workgroup
constexpr int FV = 4;                   // float4 per thread
constexpr int FTILE = FT * FV * 4;      // pixels (C*H*W elements) per workgroup
constexpr int RT = 256;                 // terms / backward workgroups
constexpr int NREG = 7;                 // gathered terms
constexpr int REG_TERMS[NREG] = {CP_PL_T_WH, CP_PL_T_OFF, CP_PL_T_HP, CP_PL_T_HP_OFFSET, CP_PL_T_SCALE, CP_PL_T_TRACKING,
                                 CP_PL_T_TRACKING_HP};

// Device view of one gathered term of one stack.
struct RegTerm {
    const float *head, *unc, *gt, *mask;
    float *ghead, *gunc;
    const int* ind;
    int mode, n, dim, elem_mask;  // n gathered entries per (b, s); mask per element (elem_mask) or per entry
    float ref[3];
};

struct Params {
    int B, S, K, HW, ns, terms, flags;
    int nhm[2];   // channels of hm / hm_hp
    int nblk[2];  // focal workgroups per image
    float weight[CP_PL_NUM_TERMS];
    float kl_kps, kl_scale;
    const float* gt_map[2];
    const int* ind;
    float* ws_part[CP_PL_MAX_STACKS][2];  // [B][S][nblk][3]
    float* ws_npos;                       // [ns][2][B][S]
    float* ws_terms;                      // [ns][T][B][S]
    float* ws_chosen;                     // [T][B]
    int* ws_choice;                       // [B]
    RegTerm reg[CP_PL_MAX_STACKS][NREG];
};

inline size_t al(size_t x) { return (x + 255) / 256 * 256; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- 1. focal forward ----
__global__ __launch_bounds__(FT) void focal_fwd_kernel(float* __restrict__ x, float* __restrict__ pc,
                                                       const float* __restrict__ gt, float* __restrict__ part, int n, int S,
                                                       int nblk) {
    __shared__ float red[FT / 64][CP_PL_MAX_S][3];
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = (size_t)b * n;
    float lp[FV * 4], ln[FV * 4];
    long long e0[FV];  // 64-bit: an image of close to 2^31 elements must not wrap the last tile's offsets
#pragma unroll
    for (int v = 0; v < FV; ++v) {
        const long long e = (long long)blk * FTILE + (v * FT + tid) * 4;
        e0[v] = e;
        if (e < n) {  // n % 4 == 0: a float4 lies wholly inside or wholly outside
            float4 l = *reinterpret_cast<const float4*>(x + base + e);
            float y[4] = {l.x, l.y, l.z, l.w}, q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                y[j] = pl_sigmoid(y[j]);
                q[j] = pl_clamp(y[j]);
                lp[v * 4 + j] = pl_focal_pos(q[j]);
                ln[v * 4 + j] = pl_focal_neg(q[j]);
            }
            *reinterpret_cast<float4*>(x + base + e) = make_float4(y[0], y[1], y[2], y[3]);
            *reinterpret_cast<float4*>(pc + base + e) = make_float4(q[0], q[1], q[2], q[3]);
        }
    }
    for (int s = 0; s < S; ++s) {
        const float* g = gt + ((size_t)b * S + s) * n;
        float4 gv[FV];
#pragma unroll
        for (int v = 0; v < FV; ++v)
            gv[v] = e0[v] < n ? *reinterpret_cast<const float4*>(g + e0[v]) : make_float4(2.f, 2.f, 2.f, 2.f);
        float pos = 0.f, neg = 0.f, cnt = 0.f;
#pragma unroll
        for (int v = 0; v < FV; ++v) {
            const float gg[4] = {gv[v].x, gv[v].y, gv[v].z, gv[v].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {  // gt == 2 (outside the tile) satisfies neither predicate
                if (gg[j] == 1.f) {
                    pos += lp[v * 4 + j];
                    cnt += 1.f;
                } else if (gg[j] < 1.f) {
                    neg += ln[v * 4 + j] * pl_focal_negw(gg[j]);
                }
            }
        }
        pos = wave_sum(pos), neg = wave_sum(neg), cnt = wave_sum(cnt);
        if (lane == 0) red[wave][s][0] = pos, red[wave][s][1] = neg, red[wave][s][2] = cnt;
    }
    __syncthreads();
    for (int i = tid; i < S * 3; i += FT) {
        const int s = i / 3, q = i - s * 3;
        float v = red[0][s][q];
#pragma unroll
        for (int w = 1; w < FT / 64; ++w) v += red[w][s][q];
        part[(((size_t)b * S + s) * nblk + blk) * 3 + q] = v;
    }
}

// fixed-order workgroup sum (RT threads); every thread gets the total
__device__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.;
#pragma unroll
    for (int w = 0; w < RT / 64; ++w) t += sh[w];
    return t;
}

// ---- 2. per (b, s, stack) terms ----
__global__ __launch_bounds__(RT) void terms_kernel(Params p) {
    __shared__ double sh[RT / 64];
    __shared__ double fsum[2][3];
    const int bs = blockIdx.x, st = blockIdx.y, b = bs / p.S, s = bs - b * p.S, tid = threadIdx.x;
    float* terms = p.ws_terms + (size_t)st * CP_PL_NUM_TERMS * p.B * p.S;
    // focal: hm [0] and hm_hp [1]
    if (tid < 6) {
        const int h = tid / 3, q = tid - h * 3;
        double v = 0.;
        if (p.ws_part[st][h]) {
            const float* pp = p.ws_part[st][h] + ((size_t)b * p.S + s) * p.nblk[h] * 3 + q;
            for (int k = 0; k < p.nblk[h]; ++k) v += pp[(size_t)k * 3];
        }
        fsum[h][q] = v;
    }
    __syncthreads();
    if (tid < 2) {
        const int h = tid, t = h == 0 ? CP_PL_T_HM : CP_PL_T_HM_HP;
        const double pos = fsum[h][0], neg = fsum[h][1], np = fsum[h][2];
        const double loss = np == 0. ? -neg : -(pos + neg) / np;  // losses.py:72-74
        terms[(size_t)t * p.B * p.S + bs] = (p.terms >> t & 1) ? (float)loss : 0.f;
        p.ws_npos[(((size_t)st * 2 + h) * p.B + b) * p.S + s] = (float)np;
    }
    // gathered terms
    for (int r = 0; r < NREG; ++r) {
        const int t = REG_TERMS[r];
        if (!(p.terms >> t & 1)) {  // uniform branch
            if (tid == 0) terms[(size_t)t * p.B * p.S + bs] = 0.f;
            continue;
        }
        const RegTerm& R = p.reg[st][r];
        const size_t row = (size_t)b * p.S + s;
        const int* ind = R.ind + row * R.n;
        const float* gt = R.gt + row * R.n * R.dim;
        const float* mk = R.mask + row * (size_t)R.n * (R.elem_mask ? R.dim : 1);
        double num = 0., den = 0.;
        for (int i = tid; i < R.n * R.dim; i += RT) {
            const int k = i / R.dim, d = i - k * R.dim;
            const int idx = ind[k];
            const bool ok = idx >= 0 && idx < p.HW;
            const size_t src = ((size_t)b * R.dim + d) * p.HW + (ok ? idx : 0);
            const float m = ok ? mk[R.elem_mask ? i : k] : 0.f;
            const float u = R.unc ? R.unc[src] : 0.f;
            num += (double)pl_reg_value<float>(R.mode, gt[i], R.head[src], m, u, R.ref[d < 3 ? d : 0],
                                               R.mode == PL_KLD_KEY ? p.kl_kps : p.kl_scale);
            den += (double)m;
        }
        num = block_sum(num, sh);
        den = block_sum(den, sh);
        if (tid == 0) terms[(size_t)t * p.B * p.S + bs] = (float)(num / (den + (double)reg_eps(R.mode)));
    }
}

// ---- 3. selection ----
__global__ __launch_bounds__(RT) void select_kernel(Params p, float* loss_out, float* stats, long long* choice,
                                                    float* terms_out) {
    const int BS = p.B * p.S;
    for (int b = threadIdx.x; b < p.B; b += RT) {
        int best = 0;
        float bv = 0.f;
        for (int s = 0; s < p.S; ++s) {
            float tot = 0.f;
            for (int t = 0; t < CP_PL_NUM_TERMS; ++t) {
                float v = 0.f;  // hm_loss += crit(...) / num_stacks, per stack in order
                for (int st = 0; st < p.ns; ++st) v += p.ws_terms[((size_t)st * CP_PL_NUM_TERMS + t) * BS + b * p.S + s] / (float)p.ns;
                if (terms_out) terms_out[(size_t)t * BS + b * p.S + s] = v;
                tot += p.weight[t] * v;  // object_pose.py:163-168, left to right
            }
            long long isum = 0;
            const int* ind = p.ind + ((size_t)b * p.S + s) * p.K;
            for (int k = 0; k < p.K; ++k) isum += ind[k];
            const bool valid = isum > 0;
            const float x = tot * (valid ? 1.f : 0.f) + (valid ? 0.f : INFINITY);
            if (s == 0) {
                bv = x;
            } else if (!(bv != bv)) {  // torch.argmin: the first NaN wins, else the first minimum
                if (x != x || x < bv) bv = x, best = s;
            }
        }
        p.ws_choice[b] = best;
        choice[b] = best;
        for (int t = 0; t < CP_PL_NUM_TERMS; ++t) {
            float v = 0.f;
            for (int st = 0; st < p.ns; ++st) v += p.ws_terms[((size_t)st * CP_PL_NUM_TERMS + t) * BS + b * p.S + best] / (float)p.ns;
            p.ws_chosen[(size_t)t * p.B + b] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float m[CP_PL_NUM_TERMS];
        float tot = 0.f;
        for (int t = 0; t < CP_PL_NUM_TERMS; ++t) {
            double a = 0.;
            for (int b = 0; b < p.B; ++b) a += p.ws_chosen[(size_t)t * p.B + b];
            m[t] = (p.terms >> t & 1) ? (float)(a / p.B) : 0.f;
            tot += p.weight[t] * m[t];
        }
        loss_out[0] = tot;
        stats[0] = tot;
        stats[1] = m[CP_PL_T_HM], stats[2] = m[CP_PL_T_HP], stats[3] = m[CP_PL_T_HM_HP], stats[4] = m[CP_PL_T_HP_OFFSET];
        stats[5] = m[CP_PL_T_WH], stats[6] = m[CP_PL_T_OFF], stats[7] = m[CP_PL_T_SCALE], stats[8] = m[CP_PL_T_TRACKING];
        stats[9] = m[CP_PL_T_TRACKING_HP];
    }
}

// ---- 4. focal backward ----
__global__ __launch_bounds__(FT) void focal_bwd_kernel(const float* __restrict__ y, const float* __restrict__ gt,
                                                       const float* __restrict__ dy, float* __restrict__ gx,
                                                       const int* __restrict__ choice, const float* __restrict__ npos,
                                                       const float* __restrict__ dloss, float wf, int n, int S) {
    // wf = 0 when the term does not count (only dy flows); dy (may be NULL) = dL/d(in-place sigmoid) from graphs built on
    // the dirtied logits tensor, chained through sigmoid as torch's sigmoid_ backward: dy * y (1 - y)
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const int s = choice[b];
    const float np = npos[(size_t)b * S + s];
    const float coef = wf == 0.f ? 0.f : dloss[0] * wf * (np == 0.f ? -1.f : -1.f / np);
    const size_t base = (size_t)b * n;
    const float* g = gt + ((size_t)b * S + s) * n;
#pragma unroll
    for (int v = 0; v < FV; ++v) {
        const long long e = (long long)blk * FTILE + (v * FT + tid) * 4;
        if (e < n) {
            const float4 yv = *reinterpret_cast<const float4*>(y + base + e);
            const float4 gv = *reinterpret_cast<const float4*>(g + e);
            float r[4] = {pl_focal_dlogit(yv.x, gv.x, coef), pl_focal_dlogit(yv.y, gv.y, coef),
                          pl_focal_dlogit(yv.z, gv.z, coef), pl_focal_dlogit(yv.w, gv.w, coef)};
            if (dy) {
                const float4 d4 = *reinterpret_cast<const float4*>(dy + base + e);
                r[0] += d4.x * (yv.x * (1.f - yv.x)), r[1] += d4.y * (yv.y * (1.f - yv.y));
                r[2] += d4.z * (yv.z * (1.f - yv.z)), r[3] += d4.w * (yv.w * (1.f - yv.w));
            }
            *reinterpret_cast<float4*>(gx + base + e) = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
}

// ---- 5. regression backward: grid (B, NREG, ns) ----
__global__ __launch_bounds__(RT) void reg_bwd_kernel(Params p, const float* __restrict__ dloss) {
    __shared__ double sh[RT / 64];
    const int b = blockIdx.x, r = blockIdx.y, st = blockIdx.z, tid = threadIdx.x;
    const int t = REG_TERMS[r];
    if (!(p.terms >> t & 1)) return;
    const RegTerm& R = p.reg[st][r];
    const int s = p.ws_choice[b];
    const size_t row = (size_t)b * p.S + s;
    const int* ind = R.ind + row * R.n;
    const float* gt = R.gt + row * R.n * R.dim;
    const float* mk = R.mask + row * (size_t)R.n * (R.elem_mask ? R.dim : 1);
    // the term's denominator for the chosen variant, summed as the forward sums it
    double den = 0.;
    for (int i = tid; i < R.n * R.dim; i += RT) {
        const int k = i / R.dim, idx = ind[k];
        den += (idx >= 0 && idx < p.HW) ? (double)mk[R.elem_mask ? i : k] : 0.;
    }
    den = block_sum(den, sh);
    const float kl = R.mode == PL_KLD_KEY ? p.kl_kps : p.kl_scale;
    const float coef = (float)((double)dloss[0] * p.weight[t] / ((double)p.B * p.ns) / (den + (double)reg_eps(R.mode)));
    const int d = tid;
    if (d >= R.dim) return;
    for (int k = 0; k < R.n; ++k) {  // serial in k: repeated indices add in entry order
        const int idx = ind[k];
        if (!(idx >= 0 && idx < p.HW)) continue;
        const int i = k * R.dim + d;
        const size_t src = ((size_t)b * R.dim + d) * p.HW + idx;
        const float m = mk[R.elem_mask ? i : k];
        const float u = R.unc ? R.unc[src] : 0.f;
        float dp, du;
        pl_reg_grad<float>(R.mode, gt[i], R.head[src], m, u, R.ref[d < 3 ? d : 0], kl, &dp, &du);
        R.ghead[src] += coef * dp;
        if (R.gunc) R.gunc[src] += coef * du;
    }
}

// ---- host side ----
struct Layout {
    size_t part[CP_PL_MAX_STACKS][2], npos, terms, chosen, choice, total;
};

int nblk_of(int n) { return (n + FTILE - 1) / FTILE; }

// the product of the extents is below 2^31 (exact in double at that size)
bool lt31(double a, double b = 1, double c = 1, double d = 1) { return a * b * c * d < 2147483648.0; }

// the heat-map kernels move float4 lines
bool al16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

bool has_maps(const cp_pose_loss_desc* d, int h) {
    return h == 0 || (d->flags & CP_PL_HM_HP_MAPS) || (d->terms >> CP_PL_T_HM_HP & 1);
}

Layout layout(const cp_pose_loss_desc* d) {
    Layout L{};
    size_t o = 0;
    const size_t HW = (size_t)d->H * d->W;
    for (int st = 0; st < d->num_stacks; ++st)
        for (int h = 0; h < 2; ++h) {
            const int ch = h == 0 ? d->num_classes : d->num_joints;
            L.part[st][h] = o;
            if (has_maps(d, h)) o += al((size_t)d->B * d->S * nblk_of((int)(ch * HW)) * 3 * 4);
        }
    L.npos = o, o += al((size_t)d->num_stacks * 2 * d->B * d->S * 4);
    L.terms = o, o += al((size_t)d->num_stacks * CP_PL_NUM_TERMS * d->B * d->S * 4);
    L.chosen = o, o += al((size_t)CP_PL_NUM_TERMS * d->B * 4);
    L.choice = o, o += al((size_t)d->B * 4);
    L.total = o;
    return L;
}

const char* check(const cp_pose_loss_desc* d) {
    if (!d) return "pose_loss: null descriptor";
    if (d->num_stacks < 1 || d->num_stacks > CP_PL_MAX_STACKS) return "pose_loss: num_stacks out of range";
    if (d->B < 1 || d->S < 1 || d->S > CP_PL_MAX_S) return "pose_loss: B or S out of range";
    if (d->K < 1 || d->K > CP_PL_MAX_K) return "pose_loss: K out of range";
    if (d->num_joints < 1 || d->num_joints > 32 || d->num_classes < 1) return "pose_loss: num_joints / num_classes out of range";
    if (d->H < 1 || d->W < 1 || ((long long)d->H * d->W) % 4) return "pose_loss: H*W must be a positive multiple of 4";
    if (d->terms & ~((1 << CP_PL_NUM_TERMS) - 1)) return "pose_loss: unknown term bits";
    if (!(d->terms >> CP_PL_T_HM & 1) || !(d->terms >> CP_PL_T_HP & 1)) return "pose_loss: hm and hp always count";
    const long long B = d->B, S = d->S, K = d->K, J = d->num_joints, HW = (long long)d->H * d->W;
    const long long maxch = std::max<long long>(std::max<long long>(d->num_classes, 2 * J),
                                              (d->terms >> CP_PL_T_SCALE & 1) ? 3 : 2);  // scale heads: 3 channels
    if (!lt31(B, S, d->num_classes, HW) || !lt31(B, S, J, HW) || !lt31(B, maxch, HW) || !lt31(B, S, K * J, 2))
        return "pose_loss: a tensor holds 2^31 elements or more";
    if (!d->gt_hm || !d->ind) return "pose_loss: null ground truth";
    if (has_maps(d, 1) && !d->gt_hm_hp) return "pose_loss: null hm_hp ground truth";
    const unsigned T = d->terms;
    if (!d->reg_mask && (T & (1 << CP_PL_T_WH | 1 << CP_PL_T_OFF | 1 << CP_PL_T_SCALE))) return "pose_loss: null reg_mask";
    if (!d->gt_hps || !d->hps_mask) return "pose_loss: null hps ground truth";
    if ((T >> CP_PL_T_WH & 1) && !d->gt_wh) return "pose_loss: null wh ground truth";
    if ((T >> CP_PL_T_OFF & 1) && !d->gt_reg) return "pose_loss: null reg ground truth";
    if ((T >> CP_PL_T_SCALE & 1) && !d->gt_scale) return "pose_loss: null scale ground truth";
    if ((T >> CP_PL_T_HP_OFFSET & 1) && (!d->hp_ind || !d->hp_mask || !d->gt_hp_offset)) return "pose_loss: null hp_offset ground truth";
    if ((T >> CP_PL_T_TRACKING & 1) && (!d->gt_tracking || !d->tracking_mask)) return "pose_loss: null tracking ground truth";
    if ((T >> CP_PL_T_TRACKING_HP & 1) && (!d->gt_tracking_hp || !d->tracking_hp_mask))
        return "pose_loss: null tracking_hp ground truth";
    if (!al16(d->gt_hm) || (has_maps(d, 1) && !al16(d->gt_hm_hp))) return "pose_loss: heat-map ground truth not 16-byte aligned";
    const bool train = !(d->flags & CP_PL_VAL);
    for (int st = 0; st < d->num_stacks; ++st) {
        float* const* h = d->head[st];
        if (!h[CP_PL_H_HM] || !d->clamped[st][0]) return "pose_loss: null hm head";
        if (has_maps(d, 1) && (!h[CP_PL_H_HM_HP] || !d->clamped[st][1])) return "pose_loss: null hm_hp head";
        if (!al16(h[CP_PL_H_HM]) || !al16(d->clamped[st][0]) ||
            (has_maps(d, 1) && (!al16(h[CP_PL_H_HM_HP]) || !al16(d->clamped[st][1]))))
            return "pose_loss: hm / hm_hp head or clamped map not 16-byte aligned";
        if (!h[CP_PL_H_HPS]) return "pose_loss: null hps head";
        if (train && (d->flags & CP_PL_HPS_UNCERTAINTY) && !h[CP_PL_H_HPS_UNC]) return "pose_loss: null hps_uncertainty head";
        if ((T >> CP_PL_T_WH & 1) && !h[CP_PL_H_WH]) return "pose_loss: null wh head";
        if ((T >> CP_PL_T_OFF & 1) && !h[CP_PL_H_REG]) return "pose_loss: null reg head";
        if ((T >> CP_PL_T_SCALE & 1) && !h[CP_PL_H_SCALE]) return "pose_loss: null scale head";
        if ((T >> CP_PL_T_SCALE & 1) && train && (d->flags & CP_PL_SCALE_UNCERTAINTY) && !h[CP_PL_H_SCALE_UNC])
            return "pose_loss: null scale_uncertainty head";
        if ((T >> CP_PL_T_HP_OFFSET & 1) && !h[CP_PL_H_HP_OFFSET]) return "pose_loss: null hp_offset head";
        if ((T >> CP_PL_T_TRACKING & 1) && !h[CP_PL_H_TRACKING]) return "pose_loss: null tracking head";
        if ((T >> CP_PL_T_TRACKING_HP & 1) && !h[CP_PL_H_TRACKING_HP]) return "pose_loss: null tracking_hp head";
    }
    return nullptr;
}

Params params(const cp_pose_loss_desc* d, void* ws, float* const* grad) {
    const Layout L = layout(d);
    char* w = (char*)ws;
    Params p{};
    p.B = d->B, p.S = d->S, p.K = d->K, p.HW = d->H * d->W, p.ns = d->num_stacks, p.terms = d->terms, p.flags = d->flags;
    p.nhm[0] = d->num_classes, p.nhm[1] = d->num_joints;
    for (int h = 0; h < 2; ++h) p.nblk[h] = nblk_of(p.nhm[h] * p.HW);
    for (int t = 0; t < CP_PL_NUM_TERMS; ++t) p.weight[t] = d->weight[t];
    p.kl_kps = d->kl_kps, p.kl_scale = d->kl_scale;
    p.gt_map[0] = d->gt_hm, p.gt_map[1] = d->gt_hm_hp;
    p.ind = d->ind;
    for (int st = 0; st < d->num_stacks; ++st)
        for (int h = 0; h < 2; ++h) p.ws_part[st][h] = has_maps(d, h) ? (float*)(w + L.part[st][h]) : nullptr;
    p.ws_npos = (float*)(w + L.npos);
    p.ws_terms = (float*)(w + L.terms);
    p.ws_chosen = (float*)(w + L.chosen);
    p.ws_choice = (int*)(w + L.choice);
    const bool train = !(d->flags & CP_PL_VAL);
    const int J = d->num_joints;
    for (int st = 0; st < d->num_stacks; ++st) {
        float* const* h = d->head[st];
        float* const* g = grad ? grad + st * CP_PL_NUM_HEADS : nullptr;
        auto set = [&](int r, int hh, int hu, const float* gt, const float* mask, const int* ind, int mode, int n, int dim,
                       int elem) {
            RegTerm& R = p.reg[st][r];
            R.head = h[hh], R.unc = hu >= 0 ? h[hu] : nullptr, R.gt = gt, R.mask = mask, R.ind = ind;
            R.ghead = g ? g[hh] : nullptr, R.gunc = (g && hu >= 0) ? g[hu] : nullptr;
            R.mode = mode, R.n = n, R.dim = dim, R.elem_mask = elem;
            for (int i = 0; i < 3; ++i) R.ref[i] = d->dimension_ref[i];
        };
        const bool kld_kps = train && (d->flags & CP_PL_HPS_UNCERTAINTY);
        set(2, CP_PL_H_HPS, kld_kps ? CP_PL_H_HPS_UNC : -1, d->gt_hps, d->hps_mask, d->ind, kld_kps ? PL_KLD_KEY : PL_L1, d->K,
            2 * J, 1);
        set(0, CP_PL_H_WH, -1, d->gt_wh, d->reg_mask, d->ind, PL_L1, d->K, 2, 0);
        set(1, CP_PL_H_REG, -1, d->gt_reg, d->reg_mask, d->ind, PL_L1, d->K, 2, 0);
        set(3, CP_PL_H_HP_OFFSET, -1, d->gt_hp_offset, d->hp_mask, d->hp_ind, PL_L1, d->K * J, 2, 0);
        const bool kld_scale = train && (d->flags & CP_PL_SCALE_UNCERTAINTY);
        const int smode = !train ? PL_L1_REL : kld_scale ? PL_KLD_SCALE : (d->flags & CP_PL_RESIDUAL) ? PL_L1_RESID : PL_L1;
        set(4, CP_PL_H_SCALE, kld_scale ? CP_PL_H_SCALE_UNC : -1, d->gt_scale, d->reg_mask, d->ind, smode, d->K, 3, 0);
        set(5, CP_PL_H_TRACKING, -1, d->gt_tracking, d->tracking_mask, d->ind, PL_L1, d->K, 2, 0);
        set(6, CP_PL_H_TRACKING_HP, -1, d->gt_tracking_hp, d->tracking_hp_mask, d->ind, PL_L1, d->K, 2 * J, 1);
    }
    return p;
}

}  // namespace

size_t cp_pose_loss_ws_bytes(const cp_pose_loss_desc* d) { return check(d) ? 0 : layout(d).total; }

const char* cp_pose_loss_check(const cp_pose_loss_desc* d) { return check(d); }

int cp_launch_pose_loss_forward(hipStream_t s, const cp_pose_loss_desc* d, float* loss, float* stats, long long* choice,
                                float* terms_out, void* ws) {
    const Params p = params(d, ws, nullptr);
    const size_t HW = (size_t)d->H * d->W;
    for (int st = 0; st < d->num_stacks; ++st)
        for (int h = 0; h < 2; ++h) {
            if (!has_maps(d, h)) continue;
            const int n = (int)(p.nhm[h] * HW);
            hipLaunchKernelGGL(focal_fwd_kernel, dim3(p.nblk[h], d->B), dim3(FT), 0, s,
                               d->head[st][h == 0 ? CP_PL_H_HM : CP_PL_H_HM_HP], d->clamped[st][h], p.gt_map[h],
                               p.ws_part[st][h], n, d->S, p.nblk[h]);
        }
    hipLaunchKernelGGL(terms_kernel, dim3(d->B * d->S, d->num_stacks), dim3(RT), 0, s, p);
    hipLaunchKernelGGL(select_kernel, dim3(1), dim3(RT), 0, s, p, loss, stats, choice, terms_out);
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}

// a heat-map pass of the backward runs when its term counts or an incoming dL/d(sigmoid) is given
bool map_bwd(const cp_pose_loss_desc* d, const float* const* dmaps, int st, int h) {
    const int t = h == 0 ? CP_PL_T_HM : CP_PL_T_HM_HP;
    return (d->terms >> t & 1) || (has_maps(d, h) && dmaps && dmaps[st * 2 + h]);
}

const char* cp_pose_loss_check_grads(const cp_pose_loss_desc* d, const float* const* dmaps, float* const* grad) {
    if (!grad) return "pose_loss_backward: null grad array";
    const bool train = !(d->flags & CP_PL_VAL);
    const unsigned T = d->terms;
    for (int st = 0; st < d->num_stacks; ++st) {
        float* const* g = grad + st * CP_PL_NUM_HEADS;
        auto need = [&](int h) { return g[h] != nullptr; };
        if (!need(CP_PL_H_HM) || !need(CP_PL_H_HPS)) return "pose_loss_backward: null hm / hps gradient";
        if (map_bwd(d, dmaps, st, 1) && !need(CP_PL_H_HM_HP)) return "pose_loss_backward: null hm_hp gradient";
        for (int h = 0; h < 2; ++h) {
            if (!map_bwd(d, dmaps, st, h)) continue;
            const float* dy = dmaps ? dmaps[st * 2 + h] : nullptr;
            if (!al16(g[h == 0 ? CP_PL_H_HM : CP_PL_H_HM_HP]) || (dy && !al16(dy)))
                return "pose_loss_backward: heat-map gradient not 16-byte aligned";
        }
        if (train && (d->flags & CP_PL_HPS_UNCERTAINTY) && !need(CP_PL_H_HPS_UNC))
            return "pose_loss_backward: null hps_uncertainty gradient";
        if ((T >> CP_PL_T_WH & 1) && !need(CP_PL_H_WH)) return "pose_loss_backward: null wh gradient";
        if ((T >> CP_PL_T_OFF & 1) && !need(CP_PL_H_REG)) return "pose_loss_backward: null reg gradient";
        if ((T >> CP_PL_T_SCALE & 1) && !need(CP_PL_H_SCALE)) return "pose_loss_backward: null scale gradient";
        if ((T >> CP_PL_T_SCALE & 1) && train && (d->flags & CP_PL_SCALE_UNCERTAINTY) && !need(CP_PL_H_SCALE_UNC))
            return "pose_loss_backward: null scale_uncertainty gradient";
        if ((T >> CP_PL_T_HP_OFFSET & 1) && !need(CP_PL_H_HP_OFFSET)) return "pose_loss_backward: null hp_offset gradient";
        if ((T >> CP_PL_T_TRACKING & 1) && !need(CP_PL_H_TRACKING)) return "pose_loss_backward: null tracking gradient";
        if ((T >> CP_PL_T_TRACKING_HP & 1) && !need(CP_PL_H_TRACKING_HP)) return "pose_loss_backward: null tracking_hp gradient";
    }
    return nullptr;
}

int cp_launch_pose_loss_backward(hipStream_t s, const cp_pose_loss_desc* d, const float* dloss, const float* const* dmaps,
                                 float* const* grad, void* ws) {
    const Params p = params(d, ws, grad);
    const size_t HW = (size_t)d->H * d->W;
    for (int st = 0; st < d->num_stacks; ++st) {
        for (int h = 0; h < 2; ++h) {
            if (!map_bwd(d, dmaps, st, h)) continue;
            const int t = h == 0 ? CP_PL_T_HM : CP_PL_T_HM_HP;
            const int n = (int)(p.nhm[h] * HW);
            const int hh = h == 0 ? CP_PL_H_HM : CP_PL_H_HM_HP;
            const float wf = (d->terms >> t & 1) ? d->weight[t] / ((float)d->B * d->num_stacks) : 0.f;
            hipLaunchKernelGGL(focal_bwd_kernel, dim3(p.nblk[h], d->B), dim3(FT), 0, s, d->head[st][hh], p.gt_map[h],
                               dmaps ? dmaps[st * 2 + h] : nullptr, grad[st * CP_PL_NUM_HEADS + hh], p.ws_choice,
                               p.ws_npos + ((size_t)st * 2 + h) * d->B * d->S, dloss, wf, n, d->S);
        }
        for (int r = 0; r < NREG; ++r) {
            if (!(d->terms >> REG_TERMS[r] & 1)) continue;
            const RegTerm& R = p.reg[st][r];
            const size_t bytes = (size_t)d->B * R.dim * HW * 4;
            if (hipMemsetAsync(R.ghead, 0, bytes, s) != hipSuccess) return CP_ERR_LAUNCH;
            if (R.gunc && hipMemsetAsync(R.gunc, 0, bytes, s) != hipSuccess) return CP_ERR_LAUNCH;
        }
    }
    hipLaunchKernelGGL(reg_bwd_kernel, dim3(d->B, NREG, d->num_stacks), dim3(RT), 0, s, p, dloss);
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}
