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
//   3. maps_kernel         pose_targets.hip's map writer (cp_launch_gauss_maps), twice: its plain form for the current
//                          frame's hm / hm_hp, and its form with peaks for pre_hm / pre_hm_hp on the input_h x input_w
//                          planes, from the lists of step 1.
// The workspace is described once, in ptk_carve (Carve, cp_common.h); it begins with cp_pose_targets' own.
#include "../../include/centerpose_hip.h"
#include "cp_common.h"
#include "pose_targets_track_common.h"

#include <cstdio>

using namespace pose_targets;

namespace {

constexpr int NCH = 1 + CP_PT_JOINTS;  // draw-list channels per image: pre_hm, then the 8 pre_hm_hp joints

struct Ws {
    void* cur;  // cp_pose_targets' own workspace
    double *timg, *pre, *curo;
    PtkPreOut* res;  // [B][Kp]
    int* counts;     // [B*NCH]
    int4* draws;     // [B*NCH][2*Kp] (x, y, r, 0)
    double* peaks;   // [B*NCH][2*Kp]
};

Ws ptk_carve(Carve& c, const cp_pose_targets_track_desc* d) {
    const size_t B = d->cur.B, Kp = d->max_pre_objs, K = d->cur.max_objs;
    Ws w;
    w.cur = c.take<char>(cp_pose_targets_ws_bytes(&d->cur));
    w.timg = c.take<double>(B * CP_PTK_IMG_STRIDE * sizeof(double));
    w.pre = c.take<double>(B * Kp * CP_PTK_PRE_STRIDE * sizeof(double));
    w.curo = c.take<double>(B * K * CP_PTK_CUR_STRIDE * sizeof(double));
    w.res = c.take<PtkPreOut>(B * Kp * sizeof(PtkPreOut));
    w.counts = c.take<int>(B * NCH * sizeof(int));
    w.draws = c.take<int4>(B * NCH * 2 * Kp * sizeof(int4));
    w.peaks = c.take<double>(B * NCH * 2 * Kp * sizeof(double));
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
    double im[CP_PT_IMG_STRIDE];
    const int npre = ptk_pre_image(img, timg, b, im);
    PtkPre r;
    for (int c = 0; c < NCH; ++c) r.draw_on[c][0] = r.draw_on[c][1] = 0;
    if (k < Kp && k < npre) {
        ptk_pre_object(im, pre + ((size_t)b * Kp + k) * CP_PTK_PRE_STRIDE, S, op, &r);
        res[(size_t)b * Kp + k] = r.o;
    }
    ptk_emit_draws(r, b, k, Kp, counts, draws, peaks);
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
    const size_t nwg = cp_gauss_maps_workgroups((size_t)d->cur.B * ((d->pre_hm ? 1 : 0) + (d->pre_hm_hp ? CP_PT_JOINTS : 0)),
                                                (size_t)d->input_w * d->input_h);
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
    Carve c{nullptr};
    ptk_carve(c, d);
    return c.off;
}

// the record copies, shared with pose_targets_track_det.hip; `v` receives where the staged records and the lists are
int cp_ptk_stage(hipStream_t s, const cp_pose_targets_track_desc* d, void* ws, cp_ptk_ws_view* v) {
    Carve c{(char*)ws};
    const Ws w = ptk_carve(c, d);
    double* img = cp_pose_targets_ws_images(&d->cur, w.cur);
    const size_t B = d->cur.B, Kp = d->max_pre_objs, K = d->cur.max_objs;
    if (hipMemcpyAsync(w.timg, d->track_images, B * CP_PTK_IMG_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(w.pre, d->pre_objects, B * Kp * CP_PTK_PRE_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) !=
            hipSuccess ||
        hipMemcpyAsync(w.curo, d->cur_objects, B * K * CP_PTK_CUR_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) !=
            hipSuccess ||
        // the current image records, which the previous-frame kernel reads too, where cp_pose_targets keeps them (its
        // launcher stages them again, with the objects)
        hipMemcpyAsync(img, d->cur.images, B * CP_PT_IMG_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
        return CP_ERR_LAUNCH;
    v->img = img, v->timg = w.timg, v->pre = w.pre;
    v->res = w.res, v->counts = w.counts, v->draws = w.draws, v->peaks = w.peaks;
    return CP_OK;
}

// the current frame's kernels and the previous frame's maps, after a previous-objects kernel has left `res` and the lists
int cp_ptk_finish(hipStream_t s, const cp_pose_targets_track_desc* d, void* ws) {
    Carve c{(char*)ws};
    const Ws w = ptk_carve(c, d);
    const int Kp = d->max_pre_objs;
    PtTrackCur tk = {};
    tk.on = 1, tk.Kp = Kp, tk.pre_hm_hp = d->pre_hm_hp, tk.tracking = d->tracking, tk.tracking_hp = d->tracking_hp;
    tk.timg = w.timg, tk.cur = w.curo, tk.pre = w.res;
    tk.out_tracking = d->out_tracking, tk.out_tracking_mask = d->out_tracking_mask;
    tk.out_tracking_hp = d->out_tracking_hp, tk.out_tracking_hp_mask = d->out_tracking_hp_mask;
    if (cp_launch_pose_targets_cur(s, &d->cur, w.cur, &tk) != CP_OK) return CP_ERR_LAUNCH;
    cp_gauss_maps_args a = {};
    a.out0 = d->out_pre_hm, a.outj = d->out_pre_hm_hp, a.W = d->input_w, a.H = d->input_h, a.images = d->cur.B;
    a.nch = (d->pre_hm ? 1 : 0) + (d->pre_hm_hp ? CP_PT_JOINTS : 0), a.ch0 = d->pre_hm ? 0 : 1, a.stride = 2 * Kp;
    a.counts = w.counts, a.draws = w.draws, a.peaks = w.peaks;
    if (a.nch) cp_launch_gauss_maps(s, a);
    return hipGetLastError() == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
}

int cp_launch_pose_targets_track(hipStream_t s, const cp_pose_targets_track_desc* d, void* ws) {
    cp_ptk_ws_view v;
    if (cp_ptk_stage(s, d, ws, &v) != CP_OK) return CP_ERR_LAUNCH;
    hipLaunchKernelGGL(pre_objects_kernel, dim3((unsigned)d->cur.B), dim3(64), 0, s, cp_ptk_opts(d), d->cur.S, d->max_pre_objs,
                       v.img, v.timg, v.pre, (PtkPreOut*)v.res, v.counts, (int4*)v.draws, v.peaks);
    return cp_ptk_finish(s, d, ws);
}
