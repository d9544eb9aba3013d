// The gradient pack of data-parallel training (cp_grad_*): every gradient of a model into one flat float32 buffer, scaled, in
// one launch whatever the number of tensors -- the buffer one all-reduce then runs over and cp_adam_step reads its gradients
// from (centerpose_amd/data_parallel.py).  The reference has torch's DataParallel do this with one copy per tensor and replica
// (trains/base_trainer.py:42-48).
// The flat layout (cp_grad_layout) is decided by the lengths alone: tensor i at a multiple of 4 floats, then n_tensors float
// flags (1: the tensor had a gradient), padded to a multiple of 4.  The table (layout: include/centerpose_hip.h) is laid out
// on the host by cp_grad_pack_table_fill: n_tensors + 1 tensor records (the last one carries the offset of the flags), then
// chunks of at most CP_ADAM_CHUNK elements that never straddle two tensors.
// grad_pack_kernel is a pure stream: one workgroup per chunk, no LDS, no atomics.  The destination of a chunk is always
// 16-byte aligned (flat is, offsets are multiples of 4 floats, chunk starts multiples of CP_ADAM_CHUNK), so where the source is
// too (CP_GRAD_VEC) a lane moves 16 bytes and a wave 8 whole 128-byte lines per instruction, all loads of a chunk issued ahead
// of its stores; the 1..3 elements past the last whole quad go one by one.  Any other source goes element by element.  A lane
// reads what it writes and nothing else, so a source that IS its destination is scaled in place; neither pointer is __restrict__
// for that reason.  The workgroups past the chunks write the flags.  Nothing at or past flat_elems is written, whatever the
// table says.
#include <cmath>

#include "op_common.h"

namespace {

constexpr int TT = 256;
constexpr int MAX_WG = 2048;          // as optim.hip: more work items than that are walked with a grid stride
constexpr int QUADS = CP_ADAM_CHUNK / 4 / TT;  // 16-byte moves of a lane per whole chunk

struct PackTensor {
    const float* src;
    long long off;
};
struct PackChunk {
    int tensor;
    unsigned start;
    int count, flags;
};
static_assert(sizeof(PackTensor) == CP_GRAD_TENSOR_BYTES && sizeof(PackChunk) == CP_GRAD_CHUNK_BYTES, "table layout");
static_assert(QUADS * 4 * TT == CP_ADAM_CHUNK, "a whole chunk is QUADS 16-byte moves per lane");
typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 scaled(f4 q, float s) { return f4{s * q.x, s * q.y, s * q.z, s * q.w}; }

__global__ __launch_bounds__(TT) void grad_pack_kernel(const PackTensor* __restrict__ T, const PackChunk* __restrict__ C, int n_tensors,
                                                       int n_chunks, float* flat, long long flat_elems, float scale) {
    const int n_items = n_chunks + (n_tensors + TT - 1) / TT;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        if (item >= n_chunks) {  // the flags
            const int i = (item - n_chunks) * TT + threadIdx.x;
            const long long at = T[n_tensors].off + i;
            if (i < n_tensors && at < flat_elems) flat[at] = T[i].src ? 1.f : 0.f;
            continue;
        }
        const PackChunk ch = C[item];
        const PackTensor t = T[ch.tensor];
        const long long base = t.off + ch.start;
        if (base < 0 || base + ch.count > flat_elems) continue;
        float* d = flat + base;
        const int nq = ch.count >> 2;
        if (ch.flags & CP_GRAD_ZERO) {
            for (int i = threadIdx.x; i < nq; i += TT) reinterpret_cast<f4*>(d)[i] = f4{0.f, 0.f, 0.f, 0.f};
            for (int i = 4 * nq + threadIdx.x; i < ch.count; i += TT) d[i] = 0.f;
            continue;
        }
        const float* g = t.src + ch.start;
        if (!(ch.flags & CP_GRAD_VEC)) {
            for (int i = threadIdx.x; i < ch.count; i += TT) d[i] = scale * g[i];
            continue;
        }
        if (ch.count == CP_ADAM_CHUNK) {
            f4 q[QUADS];
            for (int j = 0; j < QUADS; ++j) q[j] = reinterpret_cast<const f4*>(g)[j * TT + threadIdx.x];
            for (int j = 0; j < QUADS; ++j) reinterpret_cast<f4*>(d)[j * TT + threadIdx.x] = scaled(q[j], scale);
            continue;
        }
        for (int i = threadIdx.x; i < nq; i += TT) reinterpret_cast<f4*>(d)[i] = scaled(reinterpret_cast<const f4*>(g)[i], scale);
        for (int i = 4 * nq + threadIdx.x; i < ch.count; i += TT) d[i] = scale * g[i];
    }
}

thread_local char g_msg[256];

inline long long pad4(long long n) { return (n + 3) & ~3ll; }

}  // namespace

const char* cp_grad_layout(int n_tensors, const int64_t* lengths, int64_t* offsets_or_null, long long* flat_elems, long long* n_chunks) {
    if (n_tensors < 1) return "grad_pack: n_tensors must be >= 1";
    if (!lengths) return "grad_pack: null lengths";
    long long at = 0, chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (lengths[i] < 0) {
            snprintf(g_msg, sizeof g_msg, "grad_pack: tensor %d has length %lld", i, (long long)lengths[i]);
            return g_msg;
        }
        if (lengths[i] > 0x7fffffffll || at + lengths[i] > 0x7fffffffll) return "grad_pack: more than 2^31 - 1 elements in all";
        if (offsets_or_null) offsets_or_null[i] = at;
        at = pad4(at + lengths[i]);
        chunks += (lengths[i] + CP_ADAM_CHUNK - 1) / CP_ADAM_CHUNK;
    }
    if (offsets_or_null) offsets_or_null[n_tensors] = at;  // where the flags start
    at += pad4(n_tensors);
    if (at > 0x7fffffffll) return "grad_pack: more than 2^31 - 1 elements in all";
    if (flat_elems) *flat_elems = at;
    if (n_chunks) *n_chunks = chunks;
    return nullptr;
}

size_t cp_grad_pack_table_size(int n_tensors, long long n_chunks) {
    return ((size_t)n_tensors + 1) * CP_GRAD_TENSOR_BYTES + (size_t)n_chunks * CP_GRAD_CHUNK_BYTES;
}

const char* cp_grad_pack_table_fill(void* table, int n_tensors, const void* const* src, const int64_t* lengths, const int64_t* offsets) {
    PackTensor* T = (PackTensor*)table;
    PackChunk* C = (PackChunk*)((char*)table + ((size_t)n_tensors + 1) * CP_GRAD_TENSOR_BYTES);
    long long at = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (offsets[i] != at) {  // the one layout: what cp_grad_flat_offsets gives for these lengths
            snprintf(g_msg, sizeof g_msg, "grad_pack: offset %lld of tensor %d is not the layout's (%lld)", (long long)offsets[i], i, at);
            return g_msg;
        }
        if ((uintptr_t)src[i] & 3) {
            snprintf(g_msg, sizeof g_msg, "grad_pack: tensor %d has a misaligned (float32) source", i);
            return g_msg;
        }
        T[i] = PackTensor{(const float*)src[i], at};
        const int flags = !src[i] ? CP_GRAD_ZERO : ((uintptr_t)src[i] & 15) ? 0 : CP_GRAD_VEC;
        for (long long s = 0; s < lengths[i]; s += CP_ADAM_CHUNK) {
            const long long left = lengths[i] - s;
            *C++ = PackChunk{i, (unsigned)s, (int)(left < CP_ADAM_CHUNK ? left : CP_ADAM_CHUNK), flags};
        }
        at = pad4(at + lengths[i]);
    }
    if (offsets[n_tensors] != at) return "grad_pack: the offset of the flags is not the layout's";
    T[n_tensors] = PackTensor{nullptr, at};
    return nullptr;
}

// the smallest flat buffer a table of n_tensors tensors and n_chunks chunks can describe: a tensor of c chunks has more than
// (c - 1) CP_ADAM_CHUNK elements
long long cp_grad_min_flat_elems(int n_tensors, int n_chunks) {
    const long long whole = n_chunks > n_tensors ? (long long)(n_chunks - n_tensors) * CP_ADAM_CHUNK : 0;
    return whole + pad4(n_tensors);
}

int cp_launch_grad_pack(hipStream_t s, const void* table, int n_tensors, int n_chunks, float* flat, long long flat_elems, float scale) {
    const PackTensor* T = (const PackTensor*)table;
    const PackChunk* C = (const PackChunk*)((const char*)table + ((size_t)n_tensors + 1) * CP_GRAD_TENSOR_BYTES);
    const long long n_items = (long long)n_chunks + (n_tensors + TT - 1) / TT;
    const long long rounds = (n_items + MAX_WG - 1) / MAX_WG;
    hipLaunchKernelGGL(grad_pack_kernel, dim3((unsigned)((n_items + rounds - 1) / rounds)), dim3(TT), 0, s, T, C, n_tensors, n_chunks, flat,
                       flat_elems, scale);
    return launch_ok() ? CP_OK : CP_ERR_LAUNCH;
}
