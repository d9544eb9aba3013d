// The tracking task's training targets on the device (cp_pose_targets_track): Step 1 of ObjectPoseDataset.__getitem__ in
// its noise-simulation mode (datasets/dataset_combined.py:555-937, data_generation_mode == 0) for a whole batch, and the
// current frame's targets with the three places where Step 2 reads Step 1's results.  The per-object logic of the
// previous frame is in pose_targets_track_common.h; every random draw comes from the host in the records.
//
//   1. pre_objects_kernel  one wavefront per image, lane = previous object: ptk_pre_object(); leaves per object what the
//                          current frame reads (kept, id, cts_pre, pts_pre with their masks and NaNs, the chosen variant)
//                          and compacts, per (image, channel), the Gaussians to draw as (x, y, r, k) with ballots in
//                          object order, an object's own draws first and the false positives after them: no atomics.
//                          A channel's list holds up to 2 * Kp <= 128 entries; draws with k == 0 add nothing to a map of
//                          non-negative values and are dropped.
//   2. objects_kernel      pose_targets.hip's, with its PtTrackCur additions (skip, variant filter, tracking, tracking_hp)
//   3. maps_kernel         pose_targets.hip's, for the current frame's hm / hm_hp
//   4. pre_maps_kernel     maps_kernel's scheme for a peak k and rectangular input_h x input_w planes: one workgroup per
//                          (plane, band of BAND elements), the plane's list culled to the band's rows in LDS (one wavefront,
//                          two passes of 64), every element written once as the max over the covering draws of
//                          float32(k * exp(-(dx^2+dy^2) / (2 sigma^2))) with the product in float64; nontemporal float4
//                          stores, zero lines for a band without a draw, no clear pass.  A draw whose centre lies outside
//                          the map covers what draw_umich_gaussian's clipped window covers: the pixels of the map within
//                          r of it, none if there are none (utils/image.py:143-149).
#include "../../include/centerpose_hip.h"
#include "cp_common.h"
#include "pose_targets_track_common.h"

#include <cstdio>

using namespace pose_targets;

namespace {

constexpr int NCH = 1 + CP_PT_JOINTS;  // draw-list channels per image: pre_hm, then the 8 pre_hm_hp joints
constexpr int MT = 256;                // maps kernel: threads per workgroup
constexpr int BAND = MT * 4 * 2;       // maps kernel: elements per workgroup (2 float4 per thread)
constexpr int MAXD = 2 * CP_PT_MAX_OBJS;

// written once, read by a later kernel: nontemporal, as pose_targets.hip's maps (profiles/pose_targets_bench.txt)
typedef float pt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_nt(float* p, float a, float b, float c, float d) {
    const pt_f4 v = {a, b, c, d};
    __builtin_nontemporal_store(v, reinterpret_cast<pt_f4*>(p));
}

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

struct Ws {
    void* cur;  // cp_pose_targets' own workspace
    double *timg, *pre, *curo;
    PtkPreOut* res;  // [B][Kp]
    int* counts;     // [B*NCH]
    int4* draws;     // [B*NCH][2*Kp] (x, y, r, 0)
    double* peaks;   // [B*NCH][2*Kp]
    size_t bytes;
};

Ws carve(const cp_pose_targets_track_desc* d, void* ws) {
    char* p = (char*)ws;
    const size_t B = d->cur.B, Kp = d->max_pre_objs, K = d->cur.max_objs;
    Ws w;
    w.cur = p;
    p += up256(cp_pose_targets_ws_bytes(&d->cur));
    w.timg = (double*)p;
    p += up256(B * CP_PTK_IMG_STRIDE * sizeof(double));
    w.pre = (double*)p;
    p += up256(B * Kp * CP_PTK_PRE_STRIDE * sizeof(double));
    w.curo = (double*)p;
    p += up256(B * K * CP_PTK_CUR_STRIDE * sizeof(double));
    w.res = (PtkPreOut*)p;
    p += up256(B * Kp * sizeof(PtkPreOut));
    w.counts = (int*)p;
    p += up256(B * NCH * sizeof(int));
    w.draws = (int4*)p;
    p += up256(B * NCH * 2 * Kp * sizeof(int4));
    w.peaks = (double*)p;
    p += up256(B * NCH * 2 * Kp * sizeof(double));
    w.bytes = (size_t)(p - (char*)ws);
    return w;
}

}  // namespace

pose_targets::PtkOpts cp_ptk_opts(const cp_pose_targets_track_desc* d) {
    PtkOpts o;
    o.input_w = d->input_w, o.input_h = d->input_h, o.down_ratio = d->down_ratio;
    o.center_3D = d->cur.center_3D, o.pre_hm = d->pre_hm, o.pre_hm_hp = d->pre_hm_hp;
    o.hm_heat_random = d->hm_heat_random, o.hm_hp_heat_random = d->hm_hp_heat_random;
    o.tracking_label_mode = d->tracking_label_mode;
    o.hm_disturb = d->hm_disturb, o.lost_disturb = d->lost_disturb, o.fp_disturb = d->fp_disturb;
    o.hm_hp_disturb = d->hm_hp_disturb, o.hp_lost_disturb = d->hp_lost_disturb, o.hp_fp_disturb = d->hp_fp_disturb;
    return o;
}

namespace {

__global__ void __launch_bounds__(64) pre_objects_kernel(const PtkOpts op, int S, int Kp, const double* __restrict__ img,
                                                         const double* __restrict__ timg, const double* __restrict__ pre,
                                                         PtkPreOut* __restrict__ res, int* __restrict__ counts,
                                                         int4* __restrict__ draws, double* __restrict__ peaks) {
    const int b = blockIdx.x, k = threadIdx.x;
    const double* ti = timg + (size_t)b * CP_PTK_IMG_STRIDE;
    // the current image's record with the previous frame's affine and projection matrix in it
    double im[CP_PT_IMG_STRIDE];
    for (int i = 0; i < CP_PT_IMG_STRIDE; ++i) im[i] = img[(size_t)b * CP_PT_IMG_STRIDE + i];
    for (int i = 0; i < 6; ++i) im[CP_PT_IMG_TRANS + i] = ti[CP_PTK_IMG_TRANS + i];
    for (int i = 0; i < 16; ++i) im[CP_PT_IMG_PROJ + i] = ti[CP_PTK_IMG_PROJ + i];
    const int npre = (int)ti[CP_PTK_IMG_NUM_PRE];
    PtkPre r;
    for (int c = 0; c < NCH; ++c) r.draw_on[c][0] = r.draw_on[c][1] = 0;
    if (k < Kp && k < npre) {
        ptk_pre_object(im, pre + ((size_t)b * Kp + k) * CP_PTK_PRE_STRIDE, S, op, &r);
        res[(size_t)b * Kp + k] = r.o;
    }
    ptk_emit_draws(r, b, k, Kp, counts, draws, peaks);
}

__global__ void __launch_bounds__(MT) pre_maps_kernel(float* __restrict__ pre_hm, float* __restrict__ pre_hm_hp, int W, int H,
                                                      int Kp2, int ch0, int nch, int nband, const int* __restrict__ counts,
                                                      const int4* __restrict__ draws, const double* __restrict__ peaks) {
    __shared__ int4 sd[MAXD];
    __shared__ double sden[MAXD], sk[MAXD];
    __shared__ int sn;
    const int plane = blockIdx.x / nband, band = blockIdx.x - plane * nband;  // plane = b * nch + (c - ch0)
    const int b = plane / nch, c = plane - b * nch + ch0;
    const unsigned P = (unsigned)W * H;  // < 2^31 (checked): element indices within a plane stay 32-bit
    const unsigned e0 = (unsigned)band * BAND, e1 = e0 + BAND < P ? e0 + BAND : P;
    const size_t g0 = c == 0 ? (size_t)b * P : ((size_t)b * CP_PT_JOINTS + (c - 1)) * P;  // plane offset in its tensor
    float* out = (c == 0 ? pre_hm : pre_hm_hp) + g0;
    if (threadIdx.x < 64) {  // the plane's draws whose rows meet the band's: one wavefront, 64 entries per pass
        const int n = counts[b * NCH + c];
        const int ylo = (int)(e0 / W), yhi = (int)((e1 - 1) / W);
        int base = 0;
        for (int p0 = 0; p0 < n; p0 += 64) {
            const int i = p0 + threadIdx.x;
            int4 dr = make_int4(0, 0, -1, 0);
            if (i < n) dr = draws[((size_t)b * NCH + c) * Kp2 + i];
            // 64-bit: a false positive's centre may lie anywhere
            const bool v = i < n && (long long)dr.y - dr.z <= yhi && (long long)dr.y + dr.z >= ylo;
            const unsigned long long m = __ballot(v);
            if (v) {
                const int pos = base + __popcll(m & ((1ull << threadIdx.x) - 1));
                const double sigma = (double)(2 * dr.z + 1) / 6.0;
                sd[pos] = dr;
                sden[pos] = 2 * sigma * sigma;
                sk[pos] = peaks[((size_t)b * NCH + c) * Kp2 + i];
            }
            base += __popcll(m);
        }
        if (threadIdx.x == 0) sn = base;
    }
    __syncthreads();
    const int nd = sn;
    auto value = [&](int x, int y) {
        float m = 0.f;
        for (int i = 0; i < nd; ++i) {
            const int4 dr = sd[i];
            const long long dx = (long long)x - dr.x, dy = (long long)y - dr.y;
            if (dx < -dr.z || dx > dr.z || dy < -dr.z || dy > dr.z) continue;
            // inside the window (dx^2+dy^2) / (2 sigma^2) < 9, so gaussian2D's eps cut never applies
            const float g = (float)(sk[i] * exp(-((double)dx * dx + (double)dy * dy) / sden[i]));
            m = g > m ? g : m;
        }
        return m;
    };
    // float4 body on 16-byte aligned global addresses; the plane's misaligned head and tail (W*H % 4 != 0) go scalar
    const unsigned head = (unsigned)((4 - (g0 + e0) % 4) % 4);
    const unsigned a0 = e0 + head < e1 ? e0 + head : e1;
    const unsigned n4 = (e1 - a0) / 4, a1 = a0 + 4 * n4;
    if (threadIdx.x < a0 - e0) {
        const unsigned e = e0 + threadIdx.x;
        out[e] = value((int)(e % W), (int)(e / W));
    }
    if (threadIdx.x < e1 - a1) {
        const unsigned e = a1 + threadIdx.x;
        out[e] = value((int)(e % W), (int)(e / W));
    }
    if (nd == 0) {  // nothing drawn in this band: zero lines only
        for (unsigned i = threadIdx.x; i < n4; i += MT) store_nt(out + a0 + 4 * i, 0.f, 0.f, 0.f, 0.f);
        return;
    }
    for (unsigned i = threadIdx.x; i < n4; i += MT) {
        const unsigned e = a0 + 4 * i;
        int y = (int)(e / W), x = (int)(e - (unsigned)y * W);
        float v[4];
        for (int j = 0; j < 4; ++j) {
            v[j] = value(x, y);
            if (++x == W) x = 0, ++y;
        }
        store_nt(out + e, v[0], v[1], v[2], v[3]);
    }
}

thread_local char g_msg[256];

}  // namespace

const char* cp_pose_targets_track_check(const cp_pose_targets_track_desc* d) {
    if (!d) return "pose_targets_track: null descriptor";
    if (const char* e = cp_pose_targets_check(&d->cur)) return e;
    if (d->input_w < 1 || d->input_h < 1 || (long long)d->input_w * d->input_h > 0x7fffffffLL)
        return "pose_targets_track: input_w / input_h must be >= 1 and their product below 2^31";
    if (d->down_ratio < 1) return "pose_targets_track: down_ratio must be >= 1";
    if (d->max_pre_objs < 1 || d->max_pre_objs > CP_PT_MAX_OBJS) return "pose_targets_track: max_pre_objs must be in [1, 64]";
    if (!d->track_images || !d->pre_objects || !d->cur_objects) return "pose_targets_track: null record pointer";
    if ((d->pre_hm && !d->out_pre_hm) || (d->pre_hm_hp && !d->out_pre_hm_hp) ||
        (d->tracking && (!d->out_tracking || !d->out_tracking_mask)) ||
        (d->tracking_hp && (!d->out_tracking_hp || !d->out_tracking_hp_mask)))
        return "pose_targets_track: null pointer for an output the options turn on";
    if ((d->pre_hm && (uintptr_t)d->out_pre_hm % 16) || (d->pre_hm_hp && (uintptr_t)d->out_pre_hm_hp % 16))
        return "pose_targets_track: pre_hm / pre_hm_hp must be 16-byte aligned";
    const size_t P = (size_t)d->input_w * d->input_h;
    const size_t nwg = (size_t)d->cur.B * ((d->pre_hm ? 1 : 0) + (d->pre_hm_hp ? CP_PT_JOINTS : 0)) * ((P + BAND - 1) / BAND);
    if (nwg > 0x7fffffff) return "pose_targets_track: B * planes * bands exceeds the grid";
    for (int b = 0; b < d->cur.B; ++b) {
        const double n = d->track_images[(size_t)b * CP_PTK_IMG_STRIDE + CP_PTK_IMG_NUM_PRE];
        if (!(n >= 0 && n <= d->max_pre_objs) || n != (double)(int)n) {
            snprintf(g_msg, sizeof g_msg, "pose_targets_track: image %d has %g previous objects, outside [0, max_pre_objs = %d]",
                     b, n, d->max_pre_objs);
            return g_msg;
        }
        for (int k = 0; k < (int)n; ++k) {
            const double* o = d->pre_objects + ((size_t)b * d->max_pre_objs + k) * CP_PTK_PRE_STRIDE;
            const double v = o[CP_PT_OBJ_NSYM], s = o[CP_PTK_PRE_IDSYM];
            if (!(v >= 1 && v <= d->cur.S) || v != (double)(int)v) {
                snprintf(g_msg, sizeof g_msg,
                         "pose_targets_track: image %d previous object %d has %g symmetry variants, outside [1, S = %d]", b, k,
                         v, d->cur.S);
                return g_msg;
            }
            if (!(s >= 0 && s < v) || s != (double)(int)s) {
                snprintf(g_msg, sizeof g_msg,
                         "pose_targets_track: image %d previous object %d has id_symmetry_pre %g, outside [0, %d)", b, k, s,
                         (int)v);
                return g_msg;
            }
        }
    }
    return nullptr;
}

size_t cp_pose_targets_track_ws_bytes(const cp_pose_targets_track_desc* d) {
    if (!d || d->max_pre_objs < 1 || d->max_pre_objs > CP_PT_MAX_OBJS || !cp_pose_targets_ws_bytes(&d->cur)) return 0;
    return carve(d, nullptr).bytes;
}

// the record copies, shared with pose_targets_track_det.hip; `v` receives where the staged records and the lists are
int cp_ptk_stage(hipStream_t s, const cp_pose_targets_track_desc* d, void* ws, cp_ptk_ws_view* v) {
    const Ws w = carve(d, ws);
    const size_t B = d->cur.B, Kp = d->max_pre_objs, K = d->cur.max_objs;
    if (hipMemcpyAsync(w.timg, d->track_images, B * CP_PTK_IMG_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(w.pre, d->pre_objects, B * Kp * CP_PTK_PRE_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) !=
            hipSuccess ||
        hipMemcpyAsync(w.curo, d->cur_objects, B * K * CP_PTK_CUR_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) !=
            hipSuccess ||
        // the current image records, which the previous-frame kernel reads too (cp_pose_targets' layout puts them first in
        // its workspace; its launcher stages them again, with the objects)
        hipMemcpyAsync(w.cur, d->cur.images, B * CP_PT_IMG_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
        return CP_ERR_LAUNCH;
    v->img = (const double*)w.cur, v->timg = w.timg, v->pre = w.pre;
    v->res = w.res, v->counts = w.counts, v->draws = w.draws, v->peaks = w.peaks;
    return CP_OK;
}

// the current frame's kernels and the previous frame's maps, after a previous-objects kernel has left `res` and the lists
int cp_ptk_finish(hipStream_t s, const cp_pose_targets_track_desc* d, void* ws) {
    const Ws w = carve(d, ws);
    const size_t B = d->cur.B, Kp = d->max_pre_objs;
    PtTrackCur tk = {};
    tk.on = 1, tk.Kp = (int)Kp, tk.pre_hm_hp = d->pre_hm_hp, tk.tracking = d->tracking, tk.tracking_hp = d->tracking_hp;
    tk.timg = w.timg, tk.cur = w.curo, tk.pre = w.res;
    tk.out_tracking = d->out_tracking, tk.out_tracking_mask = d->out_tracking_mask;
    tk.out_tracking_hp = d->out_tracking_hp, tk.out_tracking_hp_mask = d->out_tracking_hp_mask;
    if (cp_launch_pose_targets_cur(s, &d->cur, w.cur, &tk) != CP_OK) return CP_ERR_LAUNCH;
    const int nch = (d->pre_hm ? 1 : 0) + (d->pre_hm_hp ? CP_PT_JOINTS : 0);
    if (nch) {
        const size_t P = (size_t)d->input_w * d->input_h;
        const int nband = (int)((P + BAND - 1) / BAND);
        hipLaunchKernelGGL(pre_maps_kernel, dim3((unsigned)(B * nch * nband)), dim3(MT), 0, s, d->out_pre_hm, d->out_pre_hm_hp,
                           d->input_w, d->input_h, (int)(2 * Kp), d->pre_hm ? 0 : 1, nch, nband, (const int*)w.counts,
                           (const int4*)w.draws, (const double*)w.peaks);
    }
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_pose_targets_track(hipStream_t s, const cp_pose_targets_track_desc* d, void* ws) {
    cp_ptk_ws_view v;
    if (cp_ptk_stage(s, d, ws, &v) != CP_OK) return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(pre_objects_kernel, dim3((unsigned)d->cur.B), dim3(64), 0, s, cp_ptk_opts(d), d->cur.S, d->max_pre_objs,
                       v.img, v.timg, v.pre, (PtkPreOut*)v.res, v.counts, (int4*)v.draws, v.peaks);
    return cp_ptk_finish(s, d, ws);
}
