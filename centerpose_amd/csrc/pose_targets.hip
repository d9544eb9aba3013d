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
//   2. maps_kernel     the one Gaussian map writer of the target builders (cp_launch_gauss_maps; the previous frame's
//                      pre_hm / pre_hm_hp of pose_targets_track.hip go through it too).  One workgroup per (map plane,
//                      band of BAND elements): the plane's draw list, culled to the band's rows by one wavefront, sits in
//                      LDS; every element is written exactly once (no clear pass) as the max over the draws that cover
//                      it of float32(exp(-(dx^2+dy^2) / (2 sigma^2))), sigma = (2r+1)/6 in float64 --
//                      draw_umich_gaussian's values (utils/image.py:126-150) and render_gaussians_kernel's arithmetic
//                      (post.hip).  A max does not depend on the order of the draws: bitwise deterministic.  Stores are
//                      float4 per lane (nontemporal), whole 128-byte lines wherever the plane is line-aligned, scalar
//                      for a plane's misaligned head and tail; a band without a draw stores zero lines only.
//                      Two instantiations.  <false, 64>: hm / hm_hp, R x R planes, lists of up to max_objs <= 64 draws.
//                      <true, 128>: W x H planes, lists of up to 2 * Kp <= 128 draws read in two passes of 64, each
//                      draw with a float64 peak k, the value float32(k * exp(...)) with the product in float64, and
//                      64-bit window tests, because a false positive's centre may lie anywhere.  A draw whose centre
//                      lies outside the map covers what draw_umich_gaussian's clipped window covers: the pixels of the
//                      map within r of it, none if there are none (utils/image.py:143-149).
// The workspace is described once, in pose_targets_carve (Carve, cp_common.h): the size is that function run on nullptr.
#include "../../include/centerpose_hip.h"
#include "cp_common.h"
#include "pose_targets_common.h"
#include "pose_targets_track_common.h"

#include <cstdio>
#include <type_traits>

using namespace pose_targets;

namespace {

constexpr int NCH = 1 + CP_PT_JOINTS;  // draw-list channels per image: channel 0, then the 8 joints
constexpr int MT = 256;                // map writer: threads per workgroup
constexpr int BAND = MT * 4 * 2;       // map writer: elements per workgroup (2 float4 per thread)

// The maps are written once and read by a later kernel (the loss): nontemporal stores, 47.6 us against 71.0 us for
// default-policy stores at B = 32, S = 12, 128 x 128 (profiles/pose_targets_bench.txt).
typedef float pt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_nt(float* p, float a, float b, float c, float d) {
    const pt_f4 v = {a, b, c, d};
    __builtin_nontemporal_store(v, reinterpret_cast<pt_f4*>(p));
}

struct Ws {
    double *img, *obj;
    int* counts;  // [B*S*NCH]
    int4* draws;  // [B*S*NCH][max_objs] (x, y, r, 0)
};

Ws pose_targets_carve(Carve& c, const cp_pose_targets_desc* d) {
    const size_t B = d->B, K = d->max_objs, lists = B * d->S * NCH;
    Ws w;
    w.img = c.take<double>(B * CP_PT_IMG_STRIDE * sizeof(double));
    w.obj = c.take<double>(B * K * CP_PT_OBJ_STRIDE * sizeof(double));
    w.counts = c.take<int>(lists * sizeof(int));
    w.draws = c.take<int4>(lists * K * sizeof(int4));
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

// PEAKS: a draw has a float64 peak k and its centre may lie anywhere (a false positive's), so the window tests are 64-bit;
// CAP: the most draws a list holds, 64 per culling pass.  The plain form <false, 64> pays for neither: 64-bit tests there
// cost 5 us of 47 at S = 12 (profiles/targets_refactor_ab.txt).
template <bool PEAKS, int CAP>
__global__ void __launch_bounds__(MT) maps_kernel(const cp_gauss_maps_args a, int nband) {
    typedef typename std::conditional<PEAKS, long long, int>::type win_t;
    __shared__ int4 sd[CAP];
    __shared__ double sden[CAP], sk[PEAKS ? CAP : 1];
    __shared__ int sn;
    const int W = a.W, nch = a.nch;
    const int plane = blockIdx.x / nband, band = blockIdx.x - plane * nband;  // plane = image * nch + (c - ch0)
    const int im = plane / nch, c = plane - im * nch + a.ch0;
    const unsigned P = (unsigned)W * a.H;  // < 2^31 (checked): element indices within a plane stay 32-bit
    const unsigned e0 = (unsigned)band * BAND, e1 = e0 + BAND < P ? e0 + BAND : P;
    const size_t g0 = c == 0 ? (size_t)im * P : ((size_t)im * CP_PT_JOINTS + (c - 1)) * P;  // plane offset in its tensor
    float* out = (c == 0 ? a.out0 : a.outj) + g0;
    if (threadIdx.x < 64) {  // the plane's draws whose rows meet the band's: one wavefront, 64 entries per pass
        const int n = a.counts[im * NCH + c];
        const size_t list = ((size_t)im * NCH + c) * a.stride;
        const int ylo = (int)(e0 / W), yhi = (int)((e1 - 1) / W);
        int base = 0;
        for (int p0 = 0; p0 < CAP && p0 < n; p0 += 64) {
            const int i = p0 + threadIdx.x;
            int4 dr = make_int4(0, 0, -1, 0);
            if (i < n) dr = a.draws[list + i];
            const bool v = i < n && (win_t)dr.y - dr.z <= yhi && (win_t)dr.y + dr.z >= ylo;
            const unsigned long long m = __ballot(v);
            if (v) {
                const int pos = base + __popcll(m & ((1ull << threadIdx.x) - 1));
                const double sigma = (double)(2 * dr.z + 1) / 6.0;
                sd[pos] = dr;
                sden[pos] = 2 * sigma * sigma;
                if constexpr (PEAKS) sk[pos] = a.peaks[list + i];
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
            const win_t dx = (win_t)x - dr.x, dy = (win_t)y - dr.y;
            if (dx < -dr.z || dx > dr.z || dy < -dr.z || dy > dr.z) continue;
            // inside the window (dx^2+dy^2) / (2 sigma^2) < 9, so gaussian2D's eps cut never applies
            const double e = exp(-((double)dx * dx + (double)dy * dy) / sden[i]);
            float g;
            if constexpr (PEAKS) g = (float)(sk[i] * e);
            else g = (float)e;
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
    if (nd == 0) {  // nothing drawn in this band (most of it at any S): zero lines only
        for (unsigned i = threadIdx.x; i < n4; i += MT)
            store_nt(out + a0 + 4 * i, 0.f, 0.f, 0.f, 0.f);
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
    const size_t nwg = cp_gauss_maps_workgroups((size_t)d->B * d->S * (d->hm_hp ? NCH : 1), (size_t)d->R * d->R);
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
    Carve c{nullptr};
    pose_targets_carve(c, d);
    return c.end;  // the draw lists' own end: the ABI never rounded the last region
}

double* cp_pose_targets_ws_images(const cp_pose_targets_desc* d, void* ws) {
    Carve c{(char*)ws};
    return pose_targets_carve(c, d).img;
}

size_t cp_gauss_maps_workgroups(size_t planes, size_t plane_elems) { return planes * ((plane_elems + BAND - 1) / BAND); }

// One workgroup per (map plane, band of BAND elements).  With peaks the lists hold up to 128 draws, without up to 64.
void cp_launch_gauss_maps(hipStream_t s, const cp_gauss_maps_args& a) {
    const size_t P = (size_t)a.W * a.H;
    const int nband = (int)((P + BAND - 1) / BAND);
    const dim3 grid((unsigned)cp_gauss_maps_workgroups((size_t)a.images * a.nch, P));
    if (a.peaks)
        hipLaunchKernelGGL((maps_kernel<true, 2 * CP_PT_MAX_OBJS>), grid, dim3(MT), 0, s, a, nband);
    else
        hipLaunchKernelGGL((maps_kernel<false, CP_PT_MAX_OBJS>), grid, dim3(MT), 0, s, a, nband);
}

int cp_launch_pose_targets(hipStream_t s, const cp_pose_targets_desc* d, void* ws) {
    return cp_launch_pose_targets_cur(s, d, ws, nullptr);
}

// `tk` (device pointers, or nullptr): the tracking additions of cp_pose_targets_track (pose_targets_track.hip)
int cp_launch_pose_targets_cur(hipStream_t s, const cp_pose_targets_desc* d, void* ws, const pose_targets::PtTrackCur* tk) {
    Carve c{(char*)ws};
    const Ws w = pose_targets_carve(c, d);
    PtTrackCur t = {};
    if (tk) t = *tk;
    if (hipMemcpyAsync(w.img, d->images, (size_t)d->B * CP_PT_IMG_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) !=
            hipSuccess ||
        hipMemcpyAsync(w.obj, d->objects, (size_t)d->B * d->max_objs * CP_PT_OBJ_STRIDE * sizeof(double),
                       hipMemcpyHostToDevice, s) != hipSuccess)
        return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(objects_kernel, dim3(d->B * d->S), dim3(64), 0, s, *d, (const double*)w.img,
                       (const double*)w.obj, w.counts, w.draws, t);
    cp_gauss_maps_args a = {};
    a.out0 = d->out_hm, a.outj = d->hm_hp ? d->out_hm_hp : nullptr;
    a.W = a.H = d->R, a.images = d->B * d->S, a.nch = d->hm_hp ? NCH : 1, a.ch0 = 0, a.stride = d->max_objs;
    a.counts = w.counts, a.draws = w.draws, a.peaks = nullptr;
    cp_launch_gauss_maps(s, a);
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}
