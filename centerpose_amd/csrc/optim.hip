// Gradient-norm clipping + Adam over all tensors of a param group (cp_adam_*): what trains/base_trainer.py:91-99 does with
// clip_grad_norm_(model.parameters(), 100.) and torch.optim.Adam (test.py:41), in three launches whatever the number of
// tensors, without float atomics and without a host synchronisation:
//   1. adam_sumsq_kernel     one float64 partial of sum g^2 per chunk of the table;
//   2. adam_finalize_kernel  one workgroup: the partials in table order -> total_norm, the clip coefficient, the skipped flag, the
//                            step counters and the bias corrections 1 - beta^step in float64;
//   3. adam_update_kernel    p, m, v of every chunk; g is read, never written.
// The table (layout: include/centerpose_hip.h) is laid out on the host by cp_adam_table_fill: tensor records, then chunks of
// at most CP_ADAM_CHUNK elements that never straddle two tensors.  A chunk whose tensor has p, g, m and v all 16-byte aligned
// carries CP_ADAM_VEC (chunk starts are multiples of CP_ADAM_CHUNK elements, so the chunk is aligned as its tensor is): a lane
// then moves 16 bytes per array and the 1..3 elements past the last whole quad are taken one by one by a single lane; every
// other chunk goes element by element in the same kernel.  A misaligned tensor is not peeled up to the next boundary: p, g,
// m and v may be misaligned by different amounts.
// Reproducibility: a chunk's sum depends on the chunk alone (its elements in the two_level_sum order of op_common.h: lane
// t folds items t, t + 256, ... ascending, then the eight slab lanes in order, then the 32 columns in order), the partials are
// summed in the same order in float64, and every element's update depends on that element and the group's scalars alone.
#include <cmath>

#include "op_common.h"

namespace {

constexpr int TT = 256;
constexpr int MAX_WG = 2048;  // 256 CUs x 8 resident workgroups: more chunks than that are walked with a grid stride

struct AdamTensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long n;
    int active, reserved;
};
struct AdamChunk {
    int tensor;
    unsigned start;
    int count, flags;
};
static_assert(sizeof(AdamTensor) == CP_ADAM_TENSOR_BYTES && sizeof(AdamChunk) == CP_ADAM_CHUNK_BYTES, "table layout");
typedef float f4 __attribute__((ext_vector_type(4)));

// the scalars of one step as the update consumes them: float32(1 - beta) and float32(eps) as torch hands its Python floats
// to float32 kernels; lr stays double for lr / (1 - beta1^step)
struct AdamHyper {
    double lr;
    float w1, b2, w2, eps, wd;
};

// Sum of item(0) .. item(n_items - 1) over the workgroup, every thread calling and every thread getting the result:
// two_level_sum with the items as a [slab][32] array, then its 32 columns in order.  Not two_level_sum alone, which ends with
// 32 independent sums, one per element of a slab; here the whole workgroup owns one scalar.
template <class F>
__device__ __forceinline__ double fixed_order_sum(double (&red)[TT], int n_items, F item) {
    const int el = threadIdx.x & 31;
    const double t = two_level_sum(red, true, (n_items + 31) >> 5, 0.0, [&](double acc, int s) {
        const int i = s * 32 + el;
        return i < n_items ? acc + item(i) : acc;
    });
    __syncthreads();
    if (threadIdx.x < 32) red[threadIdx.x] = t;
    __syncthreads();
    double r = red[0];
    for (int i = 1; i < 32; ++i) r += red[i];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(TT) void adam_sumsq_kernel(const AdamTensor* __restrict__ T, const AdamChunk* __restrict__ C, int n_chunks,
                                                        double* __restrict__ partial) {
    __shared__ double red[TT];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const AdamChunk ch = C[c];
        const float* __restrict__ g = T[ch.tensor].g + ch.start;
        double r;
        if (ch.flags & CP_ADAM_VEC) {
            const int nq = ch.count >> 2, rem = ch.count & 3;
            r = fixed_order_sum(red, nq + (rem ? 1 : 0), [&](int i) {
                if (i < nq) {
                    const f4 q = reinterpret_cast<const f4*>(g)[i];
                    return ((sq(q.x) + sq(q.y)) + sq(q.z)) + sq(q.w);
                }
                double a = 0.0;
                for (int j = 0; j < rem; ++j) a += sq(g[4 * nq + j]);
                return a;
            });
        } else {
            r = fixed_order_sum(red, ch.count, [&](int i) { return sq(g[i]); });
        }
        if (threadIdx.x == 0) partial[c] = r;
    }
}

__global__ __launch_bounds__(TT) void adam_finalize_kernel(const AdamTensor* __restrict__ T, int n_tensors, int n_partials,
                                                           const double* __restrict__ partial, char* __restrict__ state, double beta1,
                                                           double beta2, float max_norm, int flags, int want_norm) {
    __shared__ double red[TT];
    float norm = __builtin_nanf(""), coef = 1.f;
    if (want_norm) norm = (float)sqrt(fixed_order_sum(red, n_partials, [&](int i) { return partial[i]; }));
    if (max_norm > 0.f) {
        // torch's clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0) in float32; a NaN stays a NaN
        const float c = max_norm / (norm + 1e-6f);
        coef = c > 1.f ? 1.f : c;
    }
    const bool skip = (flags & CP_ADAM_SKIP_NONFINITE) && !isfinite(norm);
    if (threadIdx.x == 0) {
        *reinterpret_cast<float*>(state + CP_ADAM_STATE_NORM) = norm;
        *reinterpret_cast<float*>(state + CP_ADAM_STATE_COEF) = coef;
        *reinterpret_cast<int*>(state + CP_ADAM_STATE_SKIPPED) = skip ? 1 : 0;
    }
    if (skip) return;
    float* steps = reinterpret_cast<float*>(state + CP_ADAM_STATE_STEPS);
    double* bc = reinterpret_cast<double*>(state + CP_ADAM_STATE_BC(n_tensors));
    for (int i = threadIdx.x; i < n_tensors; i += TT) {
        if (!T[i].active) continue;
        const float s = steps[i] + 1.f;
        steps[i] = s;
        bc[i] = 1.0 - pow(beta1, (double)s);
        bc[n_tensors + i] = 1.0 - pow(beta2, (double)s);
    }
}

// torch's Adam for one element (amsgrad=False, maximize=False), operation by operation as its float32 kernels round:
// grad.add(p, alpha=wd), exp_avg.lerp_(grad, 1 - b1) with lerp's two forms, exp_avg_sq.mul_(b2).addcmul_(grad, grad, 1 - b2),
// denom = sqrt(v) / sqrt(bc2) + eps, p.addcdiv_(m, denom, value=-lr / bc1)
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float coef, float step_size, float bc2_sqrt,
                                         const AdamHyper& h) {
    g = coef * g;
    if (h.wd != 0.f) g = g + h.wd * p;
    const float d = g - m;
    m = h.w1 < 0.5f ? m + h.w1 * d : g - d * (1.f - h.w1);
    v = v * h.b2 + h.w2 * g * g;
    p = p - step_size * (m / (sqrtf(v) / bc2_sqrt + h.eps));
}

__global__ __launch_bounds__(TT) void adam_update_kernel(const AdamTensor* __restrict__ T, const AdamChunk* __restrict__ C, int n_chunks,
                                                         int n_tensors, const char* __restrict__ state, AdamHyper h) {
    if (*reinterpret_cast<const int*>(state + CP_ADAM_STATE_SKIPPED)) return;
    const float coef = *reinterpret_cast<const float*>(state + CP_ADAM_STATE_COEF);
    const double* bc = reinterpret_cast<const double*>(state + CP_ADAM_STATE_BC(n_tensors));
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const AdamChunk ch = C[c];
        const AdamTensor t = T[ch.tensor];
        const float step_size = (float)(h.lr / bc[ch.tensor]), bc2_sqrt = (float)sqrt(bc[n_tensors + ch.tensor]);
        float* __restrict__ p = t.p + ch.start;
        const float* __restrict__ g = t.g + ch.start;
        float* __restrict__ m = t.m + ch.start;
        float* __restrict__ v = t.v + ch.start;
        int first = 0;  // where the element-by-element walk starts
        if (ch.flags & CP_ADAM_VEC) {
            const int nq = ch.count >> 2;
            for (int i = threadIdx.x; i < nq; i += TT) {
                const f4 pq = reinterpret_cast<f4*>(p)[i], mq = reinterpret_cast<f4*>(m)[i], vq = reinterpret_cast<f4*>(v)[i];
                const f4 gq = reinterpret_cast<const f4*>(g)[i];
                float pe[4], me[4], ve[4];
                for (int j = 0; j < 4; ++j) {
                    pe[j] = pq[j], me[j] = mq[j], ve[j] = vq[j];
                    adam_one(pe[j], gq[j], me[j], ve[j], coef, step_size, bc2_sqrt, h);
                }
                reinterpret_cast<f4*>(p)[i] = f4{pe[0], pe[1], pe[2], pe[3]};
                reinterpret_cast<f4*>(m)[i] = f4{me[0], me[1], me[2], me[3]};
                reinterpret_cast<f4*>(v)[i] = f4{ve[0], ve[1], ve[2], ve[3]};
            }
            first = 4 * nq;
        }
        for (int i = first + threadIdx.x; i < ch.count; i += TT) {
            float pe = p[i], me = m[i], ve = v[i];
            adam_one(pe, g[i], me, ve, coef, step_size, bc2_sqrt, h);
            p[i] = pe;
            m[i] = me;
            v[i] = ve;
        }
    }
}

thread_local char g_msg[256];

// chunks a tensor of n elements takes
inline long long chunks_of(long long n) { return (n + CP_ADAM_CHUNK - 1) / CP_ADAM_CHUNK; }

// rounds = ceil(n_chunks / MAX_WG) passes of a grid that is as even as the chunk count allows
inline unsigned grid_for(int n_chunks) {
    const int rounds = (n_chunks + MAX_WG - 1) / MAX_WG;
    return (unsigned)((n_chunks + rounds - 1) / rounds);
}

}  // namespace

const char* cp_adam_lengths_check(int n_tensors, const int64_t* lengths, const int* active_or_null, long long* n_chunks) {
    if (n_tensors < 1) return "adam: n_tensors must be >= 1";
    if (!lengths) return "adam: null lengths";
    long long total = 0, chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (lengths[i] < 0) {
            snprintf(g_msg, sizeof g_msg, "adam: tensor %d has length %lld", i, (long long)lengths[i]);
            return g_msg;
        }
        if (active_or_null && !active_or_null[i]) continue;
        if (lengths[i] > (1ll << 31) || (total += lengths[i]) > (1ll << 31))
            return "adam: more than 2^31 elements in one call";
        chunks += chunks_of(lengths[i]);
    }
    *n_chunks = chunks;
    return nullptr;
}

size_t cp_adam_table_size(int n_tensors, long long n_chunks) {
    return (size_t)n_tensors * CP_ADAM_TENSOR_BYTES + (size_t)n_chunks * CP_ADAM_CHUNK_BYTES;
}

const char* cp_adam_table_fill(void* table, int n_tensors, const void* const* p, const void* const* g, const void* const* m,
                               const void* const* v, const int64_t* lengths, const int* active_or_null) {
    AdamTensor* T = (AdamTensor*)table;
    AdamChunk* C = (AdamChunk*)((char*)table + (size_t)n_tensors * CP_ADAM_TENSOR_BYTES);
    for (int i = 0; i < n_tensors; ++i) {
        const bool active = !active_or_null || active_or_null[i];
        if (active && lengths[i] > 0 && (!p[i] || !g[i] || !m[i] || !v[i] || (((uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i]) & 3))) {
            snprintf(g_msg, sizeof g_msg, "adam: tensor %d has a null or misaligned (float32) pointer", i);
            return g_msg;
        }
        T[i] = AdamTensor{(float*)p[i], (const float*)g[i], (float*)m[i], (float*)v[i], (long long)lengths[i], active ? 1 : 0, 0};
        if (!active) continue;
        const bool vec = !(((uintptr_t)p[i] | (uintptr_t)g[i] | (uintptr_t)m[i] | (uintptr_t)v[i]) & 15);
        for (long long s = 0; s < lengths[i]; s += CP_ADAM_CHUNK) {
            const long long left = lengths[i] - s;
            *C++ = AdamChunk{i, (unsigned)s, (int)(left < CP_ADAM_CHUNK ? left : CP_ADAM_CHUNK), vec ? CP_ADAM_VEC : 0};
        }
    }
    return nullptr;
}

size_t cp_adam_ws_bytes(int n_chunks) { return cp_engine::align_up((size_t)(n_chunks > 0 ? n_chunks : 1) * sizeof(double), 256); }

int cp_launch_adam_step(hipStream_t s, const void* table, int n_tensors, int n_chunks, double lr, double beta1, double beta2, double eps,
                        double weight_decay, double max_norm, int flags, void* state, void* ws) {
    const AdamTensor* T = (const AdamTensor*)table;
    const AdamChunk* C = (const AdamChunk*)((const char*)table + (size_t)n_tensors * CP_ADAM_TENSOR_BYTES);
    const int want_norm = max_norm > 0.0 || (flags & CP_ADAM_SKIP_NONFINITE);
    if (want_norm && n_chunks > 0)
        hipLaunchKernelGGL(adam_sumsq_kernel, dim3(grid_for(n_chunks)), dim3(TT), 0, s, T, C, n_chunks, (double*)ws);
    hipLaunchKernelGGL(adam_finalize_kernel, dim3(1), dim3(TT), 0, s, T, n_tensors, n_chunks, (const double*)ws, (char*)state, beta1,
                       beta2, max_norm > 0.0 ? (float)max_norm : 0.f, flags, want_norm);
    if (n_chunks > 0) {
        const AdamHyper h{lr, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay};
        hipLaunchKernelGGL(adam_update_kernel, dim3(grid_for(n_chunks)), dim3(TT), 0, s, T, C, n_chunks, n_tensors, (const char*)state, h);
    }
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
