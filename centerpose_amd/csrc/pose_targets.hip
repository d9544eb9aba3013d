// ObjectPose training targets on the device: what ObjectPoseDataset.__getitem__ builds for the current frame
// (datasets/dataset_combined.py:957-1130), for a whole batch and every symmetry variant, already collated to [B,S,...].
// The per-object logic is in pose_targets_common.h.
//
//   1. objects_kernel  one wavefront per (b, s), lane k = object k: the variant projection, visibility, flip, box, radius,
//                      centre and joints of pose_targets_common.h; writes every sparse slot of (b, s, k), zeros included,
//                      and compacts, per (b, s, channel), the Gaussians to draw (channel 0 = hm, 1 + j = hm_hp joint j)
//                      with a ballot in object order: no atomics.
//                      For cp_pose_targets_track (pose_targets_track.hip) a PtTrackCur argument adds the tracking task's
//                      skip and variant filter and the tracking / tracking_hp targets; all zero, it changes nothing.
//   2. maps_kernel     one workgroup per (map plane, band of BAND elements): the plane's draw list, culled to the band's
//                      rows, sits in LDS; every element of hm / hm_hp is written exactly once (no clear pass) as the max
//                      over the draws that cover it of float32(exp(-(dx^2+dy^2) / (2 sigma^2))), sigma = (2r+1)/6 in
//                      float64 -- draw_umich_gaussian's values (utils/image.py:126-150) and render_gaussians_kernel's
//                      arithmetic (post.hip).  A max does not depend on the order of the draws: bitwise deterministic.
//                      Stores are float4 per lane (nontemporal), whole 128-byte lines wherever the plane is
//                      line-aligned; a band without a draw stores zero lines only.
#include "../../include/centerpose_hip.h"
#include "cp_common.h"
#include "pose_targets_common.h"
#include "pose_targets_track_common.h"

#include <cstdio>

using namespace pose_targets;

namespace {

constexpr int NCH = 1 + CP_PT_JOINTS;  // draw-list channels per (b, s): hm, then the 8 hm_hp joints
constexpr int MT = 256;                // maps kernel: threads per workgroup
constexpr int BAND = MT * 4 * 2;       // maps kernel: elements per workgroup (2 float4 per thread)

// The maps are written once and read by a later kernel (the loss): nontemporal stores, 47.6 us against 71.0 us for
// default-policy stores at B = 32, S = 12, 128 x 128 (profiles/pose_targets_bench.txt).
typedef float pt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_nt(float* p, float a, float b, float c, float d) {
    const pt_f4 v = {a, b, c, d};
    __builtin_nontemporal_store(v, reinterpret_cast<pt_f4*>(p));
}

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

struct Ws {
    double *img, *obj;
    int* counts;  // [B*S*NCH]
    int4* draws;  // [B*S*NCH][max_objs] (x, y, r, 0)
};

Ws carve(const cp_pose_targets_desc* d, void* ws) {
    char* p = (char*)ws;
    Ws w;
    w.img = (double*)p;
    p += up256((size_t)d->B * CP_PT_IMG_STRIDE * sizeof(double));
    w.obj = (double*)p;
    p += up256((size_t)d->B * d->max_objs * CP_PT_OBJ_STRIDE * sizeof(double));
    w.counts = (int*)p;
    p += up256((size_t)d->B * d->S * NCH * sizeof(int));
    w.draws = (int4*)p;
    return w;
}

__global__ void __launch_bounds__(64) objects_kernel(cp_pose_targets_desc d, const double* __restrict__ img,
                                                     const double* __restrict__ obj, int* __restrict__ counts,
                                                     int4* __restrict__ draws, const PtTrackCur tk) {
    const int bs = blockIdx.x, b = bs / d.S, s = bs - b * d.S, k = threadIdx.x, K = d.max_objs;
    const double* im = img + (size_t)b * CP_PT_IMG_STRIDE;
    const double* ob = obj + ((size_t)b * K + (k < K ? k : 0)) * CP_PT_OBJ_STRIDE;
    const int flags = (d.center_3D ? PT_CENTER_3D : 0) | (d.use_absolute_scale ? PT_ABS_SCALE : 0);
    PtResult r;
    r.kept = 0;
    bool run = k < K && k < (int)im[CP_PT_IMG_NUM_OBJS] && s < (int)ob[CP_PT_OBJ_NSYM];
    // the tracking task (cp_pose_targets_track): the cup / mug skip (:968-972) and the variant filter (:983-987), which
    // reads the previous list at the CURRENT index k, as the reference does
    const double* cu = tk.on ? tk.cur + ((size_t)b * K + (k < K ? k : 0)) * CP_PTK_CUR_STRIDE : nullptr;
    const int npre = tk.on ? (int)tk.timg[(size_t)b * CP_PTK_IMG_STRIDE + CP_PTK_IMG_NUM_PRE] : 0;
    const PtkPreOut* pre = tk.on ? tk.pre + (size_t)b * tk.Kp : nullptr;
    if (tk.on && run) {
        if (cu[CP_PTK_CUR_SKIP] != 0.0) run = false;
        if (run && tk.pre_hm_hp && (int)ob[CP_PT_OBJ_NSYM] != 1 && k < npre && pre[k].chosen >= 0 && pre[k].chosen != s)
            run = false;
    }
    if (run) pt_object(im, ob, s, d.S, d.R, flags, &r);
    if (k < K) {
        const bool kept = r.kept != 0;
        const size_t o = (size_t)bs * K + k;
        if (tk.on) {  // the first kept previous object with this object's id (track_ids.index, :1110, :1133)
            int m = -1;
            if (kept) {
                const int id = (int)cu[CP_PTK_CUR_ID];
                for (int q = 0; q < npre && m < 0; ++q)
                    if (pre[q].kept && pre[q].id == id) m = q;
            }
            if (tk.tracking) {  // previous - current, float64, into the float32 array (:1135-1137)
                const bool has = m >= 0 && !pre[m].cts_none;
                for (int i = 0; i < 2; ++i) tk.out_tracking[2 * o + i] = has ? (float)(pre[m].cts[i] - (double)r.ct[i]) : 0.f;
                tk.out_tracking_mask[o] = has ? 1 : 0;
            }
            if (tk.tracking_hp)  // inside the joint's own block; a NaN label writes nothing (:1106-1117)
                for (int j = 0; j < CP_PT_JOINTS; ++j) {
                    bool wr = kept && r.joint_ok[j] && m >= 0;
                    if (wr) wr = !(pre[m].pts[2 * j] != pre[m].pts[2 * j]) && !(pre[m].pts[2 * j + 1] != pre[m].pts[2 * j + 1]);
                    for (int c = 0; c < 2; ++c) {
                        const size_t e = o * 2 * CP_PT_JOINTS + 2 * j + c;
                        tk.out_tracking_hp[e] = wr ? (float)((double)pre[m].pts[2 * j + c] - (double)r.pt[j][c]) : 0.f;
                        tk.out_tracking_hp_mask[e] = wr ? (unsigned char)((pre[m].pmask >> j) & 1u) : 0;
                    }
                }
        }
        d.out_reg_mask[o] = kept ? 1 : 0;
        d.out_ind[o] = kept ? r.ind : 0;
        for (int i = 0; i < 2; ++i) {
            if (d.out_wh) d.out_wh[2 * o + i] = kept ? r.wh[i] : 0.f;
            if (d.out_reg) d.out_reg[2 * o + i] = kept ? r.reg[i] : 0.f;
        }
        for (int i = 0; i < 3; ++i) {
            if (d.obj_scale) d.out_scale[3 * o + i] = kept ? r.scale[i] : 0.f;
            if (d.out_scale_uncertainty) d.out_scale_uncertainty[3 * o + i] = 0.f;  // "use 0 as the std" (:1064-1066)
        }
        for (int j = 0; j < CP_PT_JOINTS; ++j) {
            const bool ok = kept && r.joint_ok[j];
            for (int c = 0; c < 2; ++c) {
                const size_t e = o * 2 * CP_PT_JOINTS + 2 * j + c;
                d.out_hps[e] = ok ? r.hps[2 * j + c] : 0.f;
                d.out_hps_mask[e] = ok ? 1 : 0;
                if (d.hps_uncertainty) d.out_hps_uncertainty[e] = ok ? (float)r.radius : 0.f;  // hp_radius (:1092)
            }
            if (d.reg_hp_offset) {
                const size_t q = o * CP_PT_JOINTS + j;
                // pts[j, :2] - pt_int: the point was already truncated into int64, so the offset is always 0 (:1096)
                d.out_hp_offset[2 * q] = 0.f;
                d.out_hp_offset[2 * q + 1] = 0.f;
                d.out_hp_ind[q] = ok ? (long long)r.pt[j][1] * d.R + r.pt[j][0] : 0;
                d.out_hp_mask[q] = ok ? 1 : 0;
            }
        }
    }
    // draw lists, compacted in object order
    const int nch = d.hm_hp ? NCH : 1;
    const unsigned long long below = (1ull << k) - 1;
    for (int c = 0; c < nch; ++c) {
        const bool v = r.kept && (c == 0 || r.joint_ok[c - 1]);
        const unsigned long long m = __ballot(v);
        if (v) {
            const int x = c == 0 ? r.ct[0] : r.pt[c - 1][0], y = c == 0 ? r.ct[1] : r.pt[c - 1][1];
            draws[((size_t)bs * NCH + c) * K + __popcll(m & below)] = make_int4(x, y, r.radius, 0);
        }
        if (k == 0) counts[bs * NCH + c] = __popcll(m);
    }
}

__global__ void __launch_bounds__(MT) maps_kernel(float* __restrict__ hm, float* __restrict__ hm_hp, int R, int K,
                                                  int nch, int nband, const int* __restrict__ counts,
                                                  const int4* __restrict__ draws) {
    __shared__ int4 sd[64];
    __shared__ double sden[64];
    __shared__ int sn;
    const int plane = blockIdx.x / nband, band = blockIdx.x - plane * nband;  // plane = (b*S + s) * nch + c
    const int bs = plane / nch, c = plane - bs * nch;
    const unsigned P = (unsigned)R * R;  // < 2^31 (R <= 46340): element indices within a plane stay 32-bit
    const unsigned e0 = (unsigned)band * BAND, e1 = e0 + BAND < P ? e0 + BAND : P;
    const size_t g0 = c == 0 ? (size_t)bs * P : ((size_t)bs * CP_PT_JOINTS + (c - 1)) * P;  // plane offset in its tensor
    float* out = (c == 0 ? hm : hm_hp) + g0;
    if (threadIdx.x < 64) {  // the plane's draws whose rows meet the band's, compacted by one wavefront
        const int n = counts[bs * NCH + c];
        const int ylo = (int)(e0 / R), yhi = (int)((e1 - 1) / R);
        int4 dr = make_int4(0, 0, -1, 0);
        if ((int)threadIdx.x < n) dr = draws[((size_t)bs * NCH + c) * K + threadIdx.x];
        const bool v = (int)threadIdx.x < n && dr.y - dr.z <= yhi && dr.y + dr.z >= ylo;
        const unsigned long long m = __ballot(v);
        if (v) {
            const int pos = __popcll(m & ((1ull << threadIdx.x) - 1));
            const double sigma = (double)(2 * dr.z + 1) / 6.0;
            sd[pos] = dr;
            sden[pos] = 2 * sigma * sigma;
        }
        if (threadIdx.x == 0) sn = __popcll(m);
    }
    __syncthreads();
    const int nd = sn;
    auto value = [&](int x, int y) {
        float m = 0.f;
        for (int i = 0; i < nd; ++i) {
            const int4 dr = sd[i];
            const int dx = x - dr.x, dy = y - dr.y;
            if (dx < -dr.z || dx > dr.z || dy < -dr.z || dy > dr.z) continue;
            // inside the window (dx^2+dy^2) / (2 sigma^2) < 9, so gaussian2D's eps cut never applies
            const float g = (float)exp(-((double)dx * dx + (double)dy * dy) / sden[i]);
            m = g > m ? g : m;
        }
        return m;
    };
    // float4 body on 16-byte aligned global addresses; the plane's misaligned head and tail (R*R % 4 != 0) go scalar
    const unsigned head = (unsigned)((4 - (g0 + e0) % 4) % 4);
    const unsigned a0 = e0 + head < e1 ? e0 + head : e1;
    const unsigned n4 = (e1 - a0) / 4, a1 = a0 + 4 * n4;
    if (threadIdx.x < a0 - e0) {
        const unsigned e = e0 + threadIdx.x;
        out[e] = value((int)(e % R), (int)(e / R));
    }
    if (threadIdx.x < e1 - a1) {
        const unsigned e = a1 + threadIdx.x;
        out[e] = value((int)(e % R), (int)(e / R));
    }
    if (nd == 0) {  // nothing drawn in this band (most of it at any S): zero lines only
        for (unsigned i = threadIdx.x; i < n4; i += MT)
            store_nt(out + a0 + 4 * i, 0.f, 0.f, 0.f, 0.f);
        return;
    }
    for (unsigned i = threadIdx.x; i < n4; i += MT) {
        const unsigned e = a0 + 4 * i;
        int y = (int)(e / R), x = (int)(e - (unsigned)y * R);
        float v[4];
        for (int j = 0; j < 4; ++j) {
            v[j] = value(x, y);
            if (++x == R) x = 0, ++y;
        }
        store_nt(out + e, v[0], v[1], v[2], v[3]);
    }
}

thread_local char g_msg[256];

}  // namespace

const char* cp_pose_targets_check(const cp_pose_targets_desc* d) {
    if (!d) return "pose_targets: null descriptor";
    if (d->B < 1) return "pose_targets: B must be >= 1";
    if (d->S < 1) return "pose_targets: S must be >= 1";
    if (d->R < 1 || d->R > 46340) return "pose_targets: R (output_res) must be in [1, 46340]";
    if (d->max_objs < 1 || d->max_objs > CP_PT_MAX_OBJS) return "pose_targets: max_objs must be in [1, 64]";
    if (d->num_joints != CP_PT_JOINTS) return "pose_targets: num_joints must be 8";
    if (!d->images || !d->objects) return "pose_targets: null record pointer";
    if (!d->out_hm || !d->out_reg_mask || !d->out_ind || !d->out_hps || !d->out_hps_mask)
        return "pose_targets: null output pointer";
    if ((d->hm_hp && !d->out_hm_hp) || (d->hps_uncertainty && !d->out_hps_uncertainty) || (d->obj_scale && !d->out_scale) ||
        (d->reg_hp_offset && (!d->out_hp_offset || !d->out_hp_ind || !d->out_hp_mask)))
        return "pose_targets: null pointer for an output the options turn on";
    if ((uintptr_t)d->out_hm % 16 || (d->hm_hp && (uintptr_t)d->out_hm_hp % 16))
        return "pose_targets: hm / hm_hp must be 16-byte aligned";
    const size_t nwg = (size_t)d->B * d->S * (d->hm_hp ? NCH : 1) * (((size_t)d->R * d->R + BAND - 1) / BAND);
    if (nwg > 0x7fffffff) return "pose_targets: B * S * planes * bands exceeds the grid";
    for (int b = 0; b < d->B; ++b) {
        const double* im = d->images + (size_t)b * CP_PT_IMG_STRIDE;
        const double n = im[CP_PT_IMG_NUM_OBJS];
        if (!(n >= 0 && n <= d->max_objs) || n != (double)(int)n) {
            snprintf(g_msg, sizeof g_msg, "pose_targets: image %d has num_objs %g, outside [0, max_objs = %d]", b, n,
                     d->max_objs);
            return g_msg;
        }
        if (!(im[CP_PT_IMG_WIDTH] >= 1 && im[CP_PT_IMG_HEIGHT] >= 1)) {
            snprintf(g_msg, sizeof g_msg, "pose_targets: image %d has no width / height", b);
            return g_msg;
        }
        for (int k = 0; k < (int)n; ++k) {
            const double v = d->objects[((size_t)b * d->max_objs + k) * CP_PT_OBJ_STRIDE + CP_PT_OBJ_NSYM];
            if (!(v >= 1 && v <= d->S) || v != (double)(int)v) {
                snprintf(g_msg, sizeof g_msg, "pose_targets: image %d object %d has %g symmetry variants, outside [1, S = %d]",
                         b, k, v, d->S);
                return g_msg;
            }
        }
    }
    return nullptr;
}

size_t cp_pose_targets_ws_bytes(const cp_pose_targets_desc* d) {
    if (!d || d->B < 1 || d->S < 1 || d->max_objs < 1 || d->max_objs > CP_PT_MAX_OBJS) return 0;
    return up256((size_t)d->B * CP_PT_IMG_STRIDE * sizeof(double)) +
           up256((size_t)d->B * d->max_objs * CP_PT_OBJ_STRIDE * sizeof(double)) +
           up256((size_t)d->B * d->S * NCH * sizeof(int)) + (size_t)d->B * d->S * NCH * d->max_objs * sizeof(int4);
}

int cp_launch_pose_targets(hipStream_t s, const cp_pose_targets_desc* d, void* ws) {
    return cp_launch_pose_targets_cur(s, d, ws, nullptr);
}

// `tk` (device pointers, or nullptr): the tracking additions of cp_pose_targets_track (pose_targets_track.hip)
int cp_launch_pose_targets_cur(hipStream_t s, const cp_pose_targets_desc* d, void* ws, const pose_targets::PtTrackCur* tk) {
    const Ws w = carve(d, ws);
    PtTrackCur t = {};
    if (tk) t = *tk;
    if (hipMemcpyAsync(w.img, d->images, (size_t)d->B * CP_PT_IMG_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) !=
            hipSuccess ||
        hipMemcpyAsync(w.obj, d->objects, (size_t)d->B * d->max_objs * CP_PT_OBJ_STRIDE * sizeof(double),
                       hipMemcpyHostToDevice, s) != hipSuccess)
        return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(objects_kernel, dim3(d->B * d->S), dim3(64), 0, s, *d, (const double*)w.img,
                       (const double*)w.obj, w.counts, w.draws, t);
    const int nch = d->hm_hp ? NCH : 1;
    const size_t P = (size_t)d->R * d->R;
    const int nband = (int)((P + BAND - 1) / BAND);
    const size_t nwg = (size_t)d->B * d->S * nch * nband;
    hipLaunchKernelGGL(maps_kernel, dim3((unsigned)nwg), dim3(MT), 0, s, d->out_hm, d->hm_hp ? d->out_hm_hp : nullptr, d->R,
                       d->max_objs, nch, nband, (const int*)w.counts, (const int4*)w.draws);
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}
