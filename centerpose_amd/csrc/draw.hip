// The overlay (cp_draw_*): the detections drawn into the 8-bit frames where they already are, after the chain
// cp_postprocess -> cp_pnp_from_post -> cp_track_step and on its stream.  The rule a pixel is coloured by, and what is drawn
// per record, are in draw_common.h (built for the host too: tests/native/draw_host.cpp).
//
// cp_draw_primitives is two launches:
//   1. draw_compact_kernel, one workgroup per image: walks the image's P slots in order, drops what draws nothing on this
//      frame (kind 0, a coordinate or size out of range, a bounding box off the frame) and writes the survivors' slot indices,
//      in order, with their clipped bounding boxes into the workspace (a ballot prefix sum per wave, the wave totals through LDS).
//   2. draw_tile_kernel, one workgroup per TW x TH pixel tile: walks the image's compact list in chunks of TT entries, tests
//      each box against the tile, stages the primitives that meet it (in order) in LDS and evaluates them for its pixels; a
//      pixel keeps the colour of the last one that covers it.  A tile's work therefore grows with the primitives near it; what
//      it pays for the rest of the image's list is one 16-byte box test per entry, spread over the workgroup.
// A tile is one wave wide: a wave owns whole rows of 64 pixels = 192 contiguous bytes.  A row the tile covers completely goes out
// as 48 dwords (the bytes gathered across lanes), when its first byte is 4-byte aligned; any other covered pixel as three byte
// stores.  No dword is ever read, merged and written back: the neighbouring pixel may belong to another workgroup.  Uncovered
// pixels and the pad bytes of a row are never written; no atomics: the result does not depend on the launch.
#include "op_common.h"

namespace {

#include "draw_common.h"  // the rule, the font, draw_build_record (host-testable)

constexpr int TT = 256;  // threads of a workgroup = entries of a staging chunk
constexpr int TW = 64;   // tile width: one wave
constexpr int TH = 16;   // tile height: four rows per wave
constexpr int TRACK_STRIDE = 520;  // CP_TRACK_STRIDE of include/centerpose_hip.h (engine_model.h hands the name to track_common.h)

static_assert(sizeof(DrawParams) == sizeof(cp_draw_params), "cp_draw_params mirrors DrawParams field by field");

struct Entry {  // one survivor of the compaction: slot index, clipped bounding box (inclusive) as x | y << 16
    int idx, lo, hi, pad;
};
static_assert(sizeof(Entry) == 16, "entry layout");

__host__ __device__ inline size_t counts_bytes(int B) { return ((size_t)B * sizeof(int) + 255) / 256 * 256; }

// exclusive prefix of `keep` over the workgroup in thread order, and the total; s_wave [TT / 64] is rewritten (two barriers)
__device__ __forceinline__ int block_scan(bool keep, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    const int below = __popcll(m & ((1ull << lane) - 1));
    __syncthreads();  // (the previous round's readers of s_wave are done)
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = 0, sum = 0;
    for (int w = 0; w < TT / 64; ++w) {
        const int c = s_wave[w];
        if (w < wave) off += c;
        sum += c;
    }
    *total = sum;
    return off + below;
}

__global__ __launch_bounds__(TT) void draw_compact_kernel(const int* __restrict__ prims, int P, int H, int W, int* __restrict__ counts,
                                                          Entry* __restrict__ entries) {
    __shared__ int s_wave[TT / 64];
    const int b = blockIdx.x;
    const int* mine = prims + (size_t)b * P * 8;
    Entry* out = entries + (size_t)b * P;
    int base = 0;
    for (int p0 = 0; p0 < P; p0 += TT) {
        const int i = p0 + (int)threadIdx.x;
        int bb[4] = {0, 0, 0, 0};
        bool keep = false;
        if (i < P) {
            int p[8];
            for (int e = 0; e < 8; ++e) p[e] = mine[(size_t)i * 8 + e];
            keep = draw_prim_bbox(p, W, H, bb);
        }
        int total;
        const int pos = block_scan(keep, s_wave, &total);
        if (keep) out[base + pos] = Entry{i, bb[0] | bb[1] << 16, bb[2] | bb[3] << 16, 0};  // base + pos <= i < P
        base += total;
    }
    if (threadIdx.x == 0) counts[b] = base;
}

__global__ __launch_bounds__(TT) void draw_tile_kernel(unsigned char* frames, int H, int W, size_t pitch, const int* __restrict__ prims,
                                                       int P, const int* __restrict__ counts, const Entry* __restrict__ entries,
                                                       int tiles_x, int tiles_y) {
    __shared__ int s_prim[TT][8];
    __shared__ int s_wave[TT / 64];
    const int per_image = tiles_x * tiles_y;
    const int b = blockIdx.x / per_image, t = blockIdx.x - b * per_image;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int n = counts[b];
    if (n <= 0) return;  // (uniform: nothing of this image draws)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int X0 = tx * TW, Y0 = ty * TH, X1 = draw_min(X0 + TW, W) - 1, Y1 = draw_min(Y0 + TH, H) - 1;
    const int x = X0 + lane, yw = Y0 + wave * (TH / 4);
    const int* mine = prims + (size_t)b * P * 8;
    const Entry* list = entries + (size_t)b * P;
    int colour[TH / 4];
    for (int r = 0; r < TH / 4; ++r) colour[r] = -1;

    for (int c0 = 0; c0 < n; c0 += TT) {
        const int i = c0 + (int)threadIdx.x;
        bool keep = false;
        Entry e = Entry{0, 0, 0, 0};
        if (i < n) {
            e = list[i];
            const int bx0 = e.lo & 0xFFFF, by0 = e.lo >> 16, bx1 = e.hi & 0xFFFF, by1 = e.hi >> 16;
            keep = !(bx1 < X0 || bx0 > X1 || by1 < Y0 || by0 > Y1);
        }
        int total;
        const int pos = block_scan(keep, s_wave, &total);
        if (keep)
            for (int k = 0; k < 8; ++k) s_prim[pos][k] = mine[(size_t)e.idx * 8 + k];  // e.idx < P by construction
        __syncthreads();
        for (int j = 0; j < total; ++j) {
            int p[8];
            for (int k = 0; k < 8; ++k) p[k] = s_prim[j][k];  // (one address per wave: a broadcast)
            for (int r = 0; r < TH / 4; ++r)
                if (draw_covers(p, x, yw + r)) colour[r] = p[6] & 0xFFFFFF;
        }
        // (block_scan's first barrier stands between these reads of s_prim and the next chunk's writes)
    }

    for (int r = 0; r < TH / 4; ++r) {
        const int y = yw + r;
        if (y >= H) break;  // (uniform per wave)
        const int c = colour[r];
        const bool cov = x < W && c >= 0;
        unsigned char* row = frames + ((size_t)b * H + y) * pitch + (size_t)X0 * 3;
        if (__ballot(cov) == ~0ull && ((uintptr_t)row & 3) == 0) {
            // the whole 192-byte run: dword l holds bytes 4 l .. 4 l + 3, byte k = channel k % 3 of pixel k / 3
            unsigned v = 0;
            for (int j = 0; j < 4; ++j) {
                const int k = lane * 4 + j;
                const int cj = __shfl(c, (k / 3) & 63);
                v |= (unsigned)((cj >> (8 * (k % 3))) & 0xFF) << (8 * j);
            }
            if (lane < 48) reinterpret_cast<unsigned*>(row)[lane] = v;
        } else if (cov) {
            row[3 * lane + 0] = (unsigned char)(c & 0xFF);
            row[3 * lane + 1] = (unsigned char)((c >> 8) & 0xFF);
            row[3 * lane + 2] = (unsigned char)((c >> 16) & 0xFF);
        }
    }
}

__global__ __launch_bounds__(64) void draw_detections_kernel(const double* __restrict__ post, const int* __restrict__ count,
                                                             const double* __restrict__ det_pnp, const double* __restrict__ cam, int B,
                                                             int K, const DrawParams P, int* __restrict__ prims) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * K) return;
    const int b = i / K, k = i - b * K;
    int* slots = prims + (size_t)i * CP_DRAW_SLOTS * 8;
    if (k >= count[b]) {
        for (int e = 0; e < CP_DRAW_SLOTS * 8; ++e) slots[e] = 0;
        return;
    }
    const double* r = post + (size_t)i * CP_POST_STRIDE;
    const double* row = det_pnp ? det_pnp + (size_t)i * CP_PNP_STRIDE : nullptr;
    const bool solved = row && row[0] == 1.0;
    double box27[27];
    const bool axes = solved && cam && (P.show_axes || P.paper_display);
    if (axes) draw_cuboid_cam(r + 2, P.show_axes ? row + 4 : row + 28, P.show_axes ? row + 24 : row + 31, box27);
    draw_build_record(P, r[0], r + 24, solved ? row + 8 : nullptr, axes ? box27 : nullptr, cam ? cam + (size_t)b * 4 : nullptr, -1.0,
                      slots);
}

__global__ __launch_bounds__(64) void draw_tracks_kernel(const void* __restrict__ state, size_t hdr_bytes, int B, int cap,
                                                         const double* __restrict__ cam, const DrawParams P, int* __restrict__ prims) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * cap) return;
    const int b = i / cap, k = i - b * cap;
    const int* hdr = (const int*)state;
    const double* tracks = (const double*)((const char*)state + hdr_bytes);
    int* slots = prims + (size_t)i * CP_DRAW_SLOTS * 8;
    const int n = hdr[4 + 4 * b];
    const double* t = tracks + (((size_t)hdr[0] * B + b) * cap + k) * TRACK_STRIDE;
    const int flags = k < n ? (int)t[3] : 0;
    if (!(flags & 4)) {
        for (int e = 0; e < CP_DRAW_SLOTS * 8; ++e) slots[e] = 0;
        return;
    }
    draw_build_record(P, t[4], t + 4 + 24, (flags & 1) ? t + 163 : nullptr, (flags & 2) ? t + 473 : nullptr,
                      cam ? cam + (size_t)b * 4 : nullptr, t[0], slots);
}

int params_refused(const cp_draw_params* params, DrawParams* P) {
    if (!params) return cp_engine::fail(CP_ERR_INVALID, "cp_draw: null params");
    std::memcpy(P, params, sizeof(*P));
    if (P->width < 1 || P->width > CP_DRAW_MAX_DIM || P->height < 1 || P->height > CP_DRAW_MAX_DIM)
        return cp_engine::fail(CP_ERR_INVALID, "cp_draw: params width and height must be in [1, 8192]");
    return CP_OK;
}

}  // namespace

using cp_engine::fail;

size_t cp_draw_workspace_bytes(int B, int P) {
    if (B < 1 || P < 1 || P > CP_DRAW_MAX_P) return 0;
    return counts_bytes(B) + (size_t)B * P * sizeof(Entry);
}

int cp_draw_primitives(cp_stream_t stream, unsigned char* frames, int B, int H, int W, size_t pitch_bytes, const int* prims, int P,
                       void* workspace, size_t workspace_bytes) {
    if (!frames || !prims || !workspace) return fail(CP_ERR_INVALID, "cp_draw_primitives: null argument");
    if (B < 1) return fail(CP_ERR_INVALID, "cp_draw_primitives: B must be >= 1");
    if (P < 1 || P > CP_DRAW_MAX_P) return fail(CP_ERR_INVALID, "cp_draw_primitives: P must be in [1, 65536]");
    if (H < 1 || H > CP_DRAW_MAX_DIM || W < 1 || W > CP_DRAW_MAX_DIM)
        return fail(CP_ERR_INVALID, "cp_draw_primitives: H and W must be in [1, 8192]");
    if (pitch_bytes < (size_t)3 * W) return fail(CP_ERR_INVALID, "cp_draw_primitives: pitch_bytes below 3 W");
    if (workspace_bytes < cp_draw_workspace_bytes(B, P)) return fail(CP_ERR_INVALID, "cp_draw_primitives: workspace too small");
    if ((uintptr_t)workspace & 15) return fail(CP_ERR_INVALID, "cp_draw_primitives: workspace must be 16-byte aligned");
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const size_t tiles = (size_t)B * tiles_x * tiles_y;
    if (tiles > 0x7FFFFFFFu) return fail(CP_ERR_INVALID, "cp_draw_primitives: more than 2^31 - 1 tiles");
    int* counts = (int*)workspace;
    Entry* entries = (Entry*)((char*)workspace + counts_bytes(B));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(draw_compact_kernel, dim3(B), dim3(TT), 0, s, prims, P, H, W, counts, entries);
    if (!launch_ok()) return fail(CP_ERR_LAUNCH, "cp_draw_primitives: compaction launch failed");
    hipLaunchKernelGGL(draw_tile_kernel, dim3((unsigned)tiles), dim3(TT), 0, s, frames, H, W, pitch_bytes, prims, P, counts, entries,
                       tiles_x, tiles_y);
    return launch_ok() ? CP_OK : fail(CP_ERR_LAUNCH, "cp_draw_primitives: tile launch failed");
}

int cp_draw_detections(cp_stream_t stream, const double* post, const int* count, const double* det_pnp, const double* cam, int B,
                       int K, const cp_draw_params* params, int* prims) {
    if (!post || !count || !prims) return fail(CP_ERR_INVALID, "cp_draw_detections: null argument");
    if (B < 1 || K < 1 || K > 128) return fail(CP_ERR_INVALID, "cp_draw_detections: B >= 1 and K in [1, 128]");
    if ((size_t)B * K > 0x7FFFFFFFu / (CP_DRAW_SLOTS * 8)) return fail(CP_ERR_INVALID, "cp_draw_detections: B K too large");
    DrawParams P;
    if (params_refused(params, &P) != CP_OK) return CP_ERR_INVALID;
    hipLaunchKernelGGL(draw_detections_kernel, dim3((B * K + 63) / 64), dim3(64), 0, (hipStream_t)stream, post, count, det_pnp, cam, B,
                       K, P, prims);
    return launch_ok() ? CP_OK : fail(CP_ERR_LAUNCH, "cp_draw_detections: launch failed");
}

int cp_draw_tracks(cp_stream_t stream, const void* state, int B, int cap, const double* cam, const cp_draw_params* params, int* prims) {
    if (!state || !prims) return fail(CP_ERR_INVALID, "cp_draw_tracks: null argument");
    if (B < 1 || cap < 1 || cap > CP_TRACK_CAP) return fail(CP_ERR_INVALID, "cp_draw_tracks: B >= 1 and cap in [1, CP_TRACK_CAP]");
    if ((size_t)B * cap > 0x7FFFFFFFu / (CP_DRAW_SLOTS * 8)) return fail(CP_ERR_INVALID, "cp_draw_tracks: B cap too large");
    DrawParams P;
    if (params_refused(params, &P) != CP_OK) return CP_ERR_INVALID;
    const size_t hdr_bytes = cp_track_state_bytes_impl(B, cap) - (size_t)2 * B * cap * TRACK_STRIDE * sizeof(double);
    hipLaunchKernelGGL(draw_tracks_kernel, dim3((B * cap + 63) / 64), dim3(64), 0, (hipStream_t)stream, state, hdr_bytes, B, cap, cam,
                       P, prims);
    return launch_ok() ? CP_OK : fail(CP_ERR_LAUNCH, "cp_draw_tracks: launch failed");
}
