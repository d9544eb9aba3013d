// Training input images on the device: what ObjectPoseDataset._get_input builds per sample
// (datasets/dataset_combined.py:278-288: warpAffine, / 255, color_aug, normalise, HWC -> CHW) after the optional horizontal
// flip (:335-339), for N frames of differing sizes in one call, each with its own transform and colour draws.  The
// per-pixel arithmetic is in train_inputs_common.h.
//
// A workgroup owns a slab of SLAB = 1024 consecutive output pixels of one image; a thread owns 4 consecutive pixels.
//   1. grey_kernel   only over runs of images whose colour flag is set: warps the slab, sums gs = BGR2GRAY(v8 / 255) in
//                    float64 (a thread's 4 pixels in order, then a tree over the 256 threads) and stores the slab's sum.
//   2. apply_kernel  every image: a colour image's workgroup first adds the image's slab sums in a fixed order (thread t
//                    takes slabs t, t + 256, ... ascending, then the same tree) -> gs_mean = float32(sum / P); no
//                    atomics, so the mean is bitwise reproducible and does not depend on the rest of the batch.  Then it
//                    warps the slab again (the taps are in cache; an 8-bit work-space copy would cost a store and a load
//                    of 3 bytes per pixel and a second record of the layout), applies steps 2-4 and stores the three
//                    planes: one float4 per thread and plane, i.e. a wavefront writes 1 KiB of whole 128-byte lines
//                    per instruction (nontemporal: the network's stem reads them in a later kernel).  Where a plane is
//                    not 16-byte aligned (out_h * out_w % 4 != 0) the threads take pixels 256 apart and store scalars,
//                    still whole lines per instruction.
// A call without a colour image launches apply_kernel only.
#include "../../include/centerpose_hip.h"
#include "cp_common.h"
#include "train_inputs_common.h"

#include <cmath>
#include <cstdio>

using namespace train_inputs;

namespace {

constexpr int TT = 256;         // threads per workgroup
constexpr int PPT = 4;          // pixels per thread
constexpr int SLAB = TT * PPT;  // pixels per workgroup

typedef float ti_f4 __attribute__((ext_vector_type(4)));

struct Ws {
    double* rec;      // [N][CP_TI_STRIDE], the caller's records
    float* means;     // [N] gs_mean (0: no colour), at CP_TI_WS_MEANS(N)
    double* partial;  // [N][nslab] grey sums per slab
};

// the public header's CP_TI_WS_MEANS(N) restates where `means` lands: right after the records, rounded up to 256 bytes
Ws train_inputs_carve(Carve& c, size_t N, size_t nslab) {
    Ws w;
    w.rec = c.take<double>(N * CP_TI_STRIDE * sizeof(double));
    w.means = c.take<float>(N * sizeof(float));
    w.partial = c.take<double>(N * nslab * sizeof(double));
    return w;
}

inline size_t slabs(int out_h, int out_w) { return ((size_t)out_h * out_w + SLAB - 1) / SLAB; }

struct TiArgs {
    const unsigned char* frames;
    const double* rec;
    float* out;
    int OW, nslab;
    unsigned P;  // out_h * out_w < 2^31 - SLAB: pixel indices stay 32-bit
    float mean[3], std[3];
    float* means;
    double* partial;
};

// thread 0 decodes the image's record (one float64 division and the inverse's products) for the workgroup
__device__ __forceinline__ void load_image(const double* __restrict__ rec, int n, TiImage* sim) {
    if (threadIdx.x == 0) ti_decode(rec + (size_t)n * CP_TI_STRIDE, sim);
    __syncthreads();
}

// sum over the workgroup in a fixed order; every thread calls it, every thread gets the result
__device__ __forceinline__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = TT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(TT) ti_grey_kernel(TiArgs a, int n0) {
    __shared__ TiImage sim;
    __shared__ double red[TT];
    const int n = n0 + blockIdx.x / a.nslab, slab = blockIdx.x % a.nslab;
    load_image(a.rec, n, &sim);
    const unsigned char* img = a.frames + sim.offset;
    const unsigned e0 = (unsigned)slab * SLAB + PPT * threadIdx.x;
    int y = (int)(e0 / a.OW), x = (int)(e0 - (unsigned)y * a.OW);
    double sum = 0.0;
    for (int j = 0; j < PPT; ++j) {
        if (e0 + j < a.P) {
            float v[3];
            sum += (double)ti_pixel(img, &sim, x, y, v);
        }
        if (++x == a.OW) x = 0, ++y;
    }
    sum = block_sum(sum, red);
    if (threadIdx.x == 0) a.partial[(size_t)n * a.nslab + slab] = sum;
}

template <bool VEC>
__global__ void __launch_bounds__(TT) ti_apply_kernel(TiArgs a) {
    __shared__ TiImage sim;
    __shared__ double red[TT];
    const int n = blockIdx.x / a.nslab, slab = blockIdx.x % a.nslab;
    load_image(a.rec, n, &sim);
    float gs_mean = 0.f;
    if (sim.color) {  // uniform over the workgroup
        double sum = 0.0;
        for (int s = threadIdx.x; s < a.nslab; s += TT) sum += a.partial[(size_t)n * a.nslab + s];
        gs_mean = (float)(block_sum(sum, red) / (double)a.P);
    }
    if (slab == 0 && threadIdx.x == 0) a.means[n] = gs_mean;
    const unsigned char* img = a.frames + sim.offset;
    float* out = a.out + (size_t)n * 3 * a.P;
    // VEC: 4 consecutive pixels per thread; else pixel j of thread t is t + 256 j of the slab
    const unsigned e0 = (unsigned)slab * SLAB + (VEC ? PPT * threadIdx.x : threadIdx.x);
    constexpr unsigned STEP = VEC ? 1 : TT;
    float r[3][PPT];
    for (int j = 0; j < PPT; ++j) {
        const unsigned e = e0 + j * STEP;
        float v[3] = {0.f, 0.f, 0.f};
        if (e < a.P) {
            const int y = (int)(e / a.OW), x = (int)(e - (unsigned)y * a.OW);
            const float gs = ti_pixel(img, &sim, x, y, v);
            if (sim.color) ti_color(v, gs, gs_mean, &sim);
            for (int c = 0; c < 3; ++c) v[c] = ti_normalise(v[c], a.mean[c], a.std[c]);
        }
        for (int c = 0; c < 3; ++c) r[c][j] = v[c];
    }
    if (VEC) {  // P % 4 == 0: a thread's 4 pixels are inside the plane together or not at all
        if (e0 < a.P)
            for (int c = 0; c < 3; ++c) {
                const ti_f4 q = {r[c][0], r[c][1], r[c][2], r[c][3]};
                __builtin_nontemporal_store(q, reinterpret_cast<ti_f4*>(out + (size_t)c * a.P + e0));
            }
    } else {
        for (int j = 0; j < PPT; ++j)
            if (e0 + j * STEP < a.P)
                for (int c = 0; c < 3; ++c) __builtin_nontemporal_store(r[c][j], out + (size_t)c * a.P + e0 + j * STEP);
    }
}

thread_local char g_msg[256];

}  // namespace

const char* cp_train_inputs_check(const unsigned char* frames, size_t frames_bytes, const double* records, int N,
                                  const float* mean3, const float* std3, const float* out, int out_h, int out_w) {
    if (!frames || !records || !mean3 || !std3 || !out) return "train_inputs: null pointer";
    if (N < 1) return "train_inputs: N must be >= 1";
    if (out_h < 1 || out_w < 1) return "train_inputs: out_h and out_w must be >= 1";
    if (!cp_train_inputs_ws_bytes(N, out_h, out_w)) return "train_inputs: N * out_h * out_w exceeds the grid";
    if ((uintptr_t)out % 16) return "train_inputs: out must be 16-byte aligned";
    for (int n = 0; n < N; ++n) {
        const double* r = records + (size_t)n * CP_TI_STRIDE;
        for (int i = 0; i < CP_TI_SHIFT + 3; ++i)
            if (!std::isfinite(r[i])) {
                snprintf(g_msg, sizeof g_msg, "train_inputs: image %d has a non-finite record value at %d", n, i);
                return g_msg;
            }
        const double H = r[CP_TI_HEIGHT], W = r[CP_TI_WIDTH], off = r[CP_TI_OFFSET], ord = r[CP_TI_ORDER];
        if (!(H >= 1 && W >= 1 && H <= 2147483647.0 && W <= 2147483647.0) || H != floor(H) || W != floor(W)) {
            snprintf(g_msg, sizeof g_msg, "train_inputs: image %d has height %g, width %g: integers >= 1 expected", n, H, W);
            return g_msg;
        }
        if (!(ord >= 0 && ord <= 5) || ord != floor(ord)) {
            snprintf(g_msg, sizeof g_msg, "train_inputs: image %d has order code %g, outside 0..5", n, ord);
            return g_msg;
        }
        // exact in float64 up to 2^53 bytes
        if (!(off >= 0) || off != floor(off) || off + 3.0 * H * W > (double)frames_bytes) {
            snprintf(g_msg, sizeof g_msg, "train_inputs: image %d's frame [%g, %g) lies outside the frames buffer of %zu bytes",
                     n, off, off + 3.0 * H * W, frames_bytes);
            return g_msg;
        }
    }
    return nullptr;
}

size_t cp_train_inputs_ws_bytes(int N, int out_h, int out_w) {
    if (N < 1 || out_h < 1 || out_w < 1) return 0;
    const size_t P = (size_t)out_h * out_w;
    if (P > 0x7fffffffull - SLAB) return 0;
    const size_t nslab = slabs(out_h, out_w);
    if ((size_t)N * nslab > 0x7fffffffull) return 0;
    Carve c{nullptr};
    train_inputs_carve(c, N, nslab);
    return c.end;  // the slab sums' own end: the ABI never rounded the last region
}

int cp_launch_train_inputs(hipStream_t s, const unsigned char* frames, const double* records, int N, const float* mean3,
                           const float* std3, float* out, int out_h, int out_w, void* ws) {
    Carve c{(char*)ws};
    const Ws w = train_inputs_carve(c, N, slabs(out_h, out_w));
    if (hipMemcpyAsync(w.rec, records, (size_t)N * CP_TI_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
        return CP_ERR_LAUNCH;
    TiArgs a;
    a.frames = frames, a.rec = w.rec, a.out = out, a.OW = out_w;
    a.P = (unsigned)((size_t)out_h * out_w);
    a.nslab = (int)slabs(out_h, out_w);
    for (int c = 0; c < 3; ++c) a.mean[c] = mean3[c], a.std[c] = std3[c];
    a.means = w.means, a.partial = w.partial;
    // the grey pass, once per run of consecutive colour images (a training batch is one run, or none)
    for (int n0 = 0; n0 < N;) {
        if (records[(size_t)n0 * CP_TI_STRIDE + CP_TI_COLOR] == 0.0) {
            ++n0;
            continue;
        }
        int n1 = n0 + 1;
        while (n1 < N && records[(size_t)n1 * CP_TI_STRIDE + CP_TI_COLOR] != 0.0) ++n1;
        hipLaunchKernelGGL(ti_grey_kernel, dim3((unsigned)(n1 - n0) * a.nslab), dim3(TT), 0, s, a, n0);
        n0 = n1;
    }
    const unsigned nwg = (unsigned)N * a.nslab;
    if (a.P % 4 == 0)
        hipLaunchKernelGGL(ti_apply_kernel<true>, dim3(nwg), dim3(TT), 0, s, a);
    else
        hipLaunchKernelGGL(ti_apply_kernel<false>, dim3(nwg), dim3(TT), 0, s, a);
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}
