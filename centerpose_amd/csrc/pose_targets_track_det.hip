// The tracking task's training targets with the detector in the loop (cp_pose_targets_track_det): a batch in which some
// images take the previous frame's heat-maps and tracking labels from a trained CenterPose detector's boxes
// (datasets/dataset_combined.py, data_generation_mode == 1) and the others from simulated noise, as
// cp_pose_targets_track builds them.  The detector's device records (cp_postprocess, cp_pnp_from_post) are read where
// they are; the per-slot and per-object logic is in pose_targets_track_det_common.h.
//
//   1. det_boxes_match_kernel   one wavefront per mode-1 image.  Lane = previous object: its instances_2d entry into LDS.
//                               Lane = detection slot, two passes of 64: is the slot a box (PnP status, pnp_shell's rejects),
//                               its norms to every object and their first minimum, left in LDS; a ballot per pass finds the
//                               image's last box.  Lane = previous object again: the box among those whose minimum it is, and
//                               the match record.  No atomics; the order of every choice is the reference's.
//   2. pre_objects_det_kernel   pose_targets_track.hip's pre_objects_kernel with ptk_pre_object_det for the mode-1 images;
//                               a mode-0 image runs ptk_pre_object, the same code as there.
//   3. cp_ptk_finish            the current frame's kernels and the map writer (pose_targets.hip's maps_kernel), unchanged.
// The workspace is described once, in ptkd_carve (Carve, cp_common.h); it begins with cp_pose_targets_track's own.
#include "../../include/centerpose_hip.h"
#include "cp_common.h"
#include "pose_targets_track_det_common.h"

#include <cmath>
#include <cstdio>

using namespace pose_targets;

namespace {

struct DetWs {
    void* track;    // cp_pose_targets_track's own workspace
    double* gen;    // [B][CP_PTKD_GEN_STRIDE]
    double* match;  // [B][Kp][PTKD_STRIDE]
};

DetWs ptkd_carve(Carve& c, const cp_pose_targets_track_det_desc* d) {
    const size_t B = d->track.cur.B, Kp = d->track.max_pre_objs;
    DetWs w;
    w.track = c.take<char>(cp_pose_targets_track_ws_bytes(&d->track));
    w.gen = c.take<double>(B * CP_PTKD_GEN_STRIDE * sizeof(double));
    w.match = c.take<double>(B * Kp * PTKD_STRIDE * sizeof(double));
    return w;
}

__global__ void __launch_bounds__(64) det_boxes_match_kernel(int Kp, int K_det, int cat_rule, const double* __restrict__ img,
                                                             const double* __restrict__ timg, const double* __restrict__ pre,
                                                             const double* __restrict__ gen, const double* __restrict__ post,
                                                             const int* __restrict__ count, const double* __restrict__ pnp,
                                                             double* __restrict__ match) {
    __shared__ double s_inst[CP_PT_MAX_OBJS][16];
    __shared__ int s_amin[CP_PTKD_MAX_K];
    __shared__ double s_nmin[CP_PTKD_MAX_K];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (gen[(size_t)b * CP_PTKD_GEN_STRIDE + CP_PTKD_GEN_MODE] == 0.0) return;  // the whole wavefront
    const double* im = img + (size_t)b * CP_PT_IMG_STRIDE;
    const double width = im[CP_PT_IMG_WIDTH], height = im[CP_PT_IMG_HEIGHT];
    int npre = (int)timg[(size_t)b * CP_PTK_IMG_STRIDE + CP_PTK_IMG_NUM_PRE];
    npre = npre < Kp ? npre : Kp;
    if (lane < npre) ptkd_instance(im, pre + ((size_t)b * Kp + lane) * CP_PTK_PRE_STRIDE, s_inst[lane]);
    __syncthreads();
    int n = count[b];
    n = n < 0 ? 0 : (n > K_det ? K_det : n);
    const double* post_b = post + (size_t)b * K_det * CP_POST_STRIDE;
    const double* pnp_b = pnp + (size_t)b * K_det * CP_PNP_STRIDE;
    int last = -1;
    for (int p0 = 0; p0 < CP_PTKD_MAX_K; p0 += 64) {
        const int k = p0 + lane;
        double p9[18];
        int am = -1;
        double nm = 0.0;
        const bool box = k < n && ptkd_box(cat_rule, width, height, pnp_b + (size_t)k * CP_PNP_STRIDE, p9);
        if (box)
            for (int o = 0; o < npre; ++o) {
                const double v = ptkd_norm(s_inst[o], p9);
                if (o == 0 || ptkd_takes(v, nm)) am = o, nm = v;
            }
        s_amin[k] = am, s_nmin[k] = nm;
        const unsigned long long m = __ballot(box);
        if (m) last = p0 + 63 - __clzll((long long)m);
    }
    __syncthreads();
    if (lane >= npre) return;
    const double last_score = last >= 0 ? post_b[(size_t)last * CP_POST_STRIDE + PO_SCORE] : 0.0;
    double norm;
    const int s = ptkd_select(s_amin, s_nmin, CP_PTKD_MAX_K, lane, &norm);
    const size_t at = (size_t)(s < 0 ? 0 : s);
    ptkd_fill(s, norm, last_score, cat_rule, width, height, post_b + at * CP_POST_STRIDE, pnp_b + at * CP_PNP_STRIDE,
              match + ((size_t)b * Kp + lane) * PTKD_STRIDE);
}

__global__ void __launch_bounds__(64) pre_objects_det_kernel(const PtkOpts op, const PtkDetOpts dop, int S, int Kp,
                                                             const double* __restrict__ img, const double* __restrict__ timg,
                                                             const double* __restrict__ pre, const double* __restrict__ gen,
                                                             const double* __restrict__ match, PtkPreOut* __restrict__ res,
                                                             int* __restrict__ counts, int4* __restrict__ draws,
                                                             double* __restrict__ peaks) {
    const int b = blockIdx.x, k = threadIdx.x;
    double im[CP_PT_IMG_STRIDE];
    const int npre = ptk_pre_image(img, timg, b, im);
    const double* gb = gen + (size_t)b * CP_PTKD_GEN_STRIDE;
    PtkPre r;
    for (int c = 0; c < 1 + CP_PT_JOINTS; ++c) r.draw_on[c][0] = r.draw_on[c][1] = 0;
    if (k < Kp && k < npre) {
        const double* po = pre + ((size_t)b * Kp + k) * CP_PTK_PRE_STRIDE;
        if (gb[CP_PTKD_GEN_MODE] == 0.0) ptk_pre_object(im, po, S, op, &r);
        else ptk_pre_object_det(im, po, match + ((size_t)b * Kp + k) * PTKD_STRIDE, gb[CP_PTKD_GEN_RADIUS_SCALE], S, op, dop, &r);
        res[(size_t)b * Kp + k] = r.o;
    }
    ptk_emit_draws(r, b, k, Kp, counts, draws, peaks);
}

thread_local char g_msg[256];

}  // namespace

const char* cp_pose_targets_track_det_check(const cp_pose_targets_track_det_desc* d) {
    if (!d) return "pose_targets_track_det: null descriptor";
    if (const char* e = cp_pose_targets_track_check(&d->track)) return e;
    if (!d->det_post || !d->det_count || !d->det_pnp) return "pose_targets_track_det: null detector record pointer";
    if (!d->gen) return "pose_targets_track_det: null gen record pointer";
    if ((uintptr_t)d->det_post % 8 || (uintptr_t)d->det_pnp % 8 || (uintptr_t)d->det_count % 4)
        return "pose_targets_track_det: det_post / det_pnp must be 8-byte and det_count 4-byte aligned";
    if (d->K_det < 1 || d->K_det > CP_PTKD_MAX_K) return "pose_targets_track_det: K_det must be in [1, 128]";
    if (d->render_hm_mode < 0 || d->render_hm_mode > 1) return "pose_targets_track_det: render_hm_mode must be 0 or 1";
    if (d->render_hmhp_mode < 0 || d->render_hmhp_mode > 3) return "pose_targets_track_det: render_hmhp_mode must be in [0, 3]";
    if (d->cat_rule < 0 || d->cat_rule > 2) return "pose_targets_track_det: cat_rule must be in [0, 2]";
    for (int b = 0; b < d->track.cur.B; ++b) {
        const double* g = d->gen + (size_t)b * CP_PTKD_GEN_STRIDE;
        if (g[CP_PTKD_GEN_MODE] != 0.0 && g[CP_PTKD_GEN_MODE] != 1.0) {
            snprintf(g_msg, sizeof g_msg, "pose_targets_track_det: image %d has data generation mode %g, not 0 or 1", b,
                     g[CP_PTKD_GEN_MODE]);
            return g_msg;
        }
        if (!std::isfinite(g[CP_PTKD_GEN_RADIUS_SCALE])) {
            snprintf(g_msg, sizeof g_msg, "pose_targets_track_det: image %d has a radius scale that is not finite", b);
            return g_msg;
        }
    }
    return nullptr;
}

size_t cp_pose_targets_track_det_ws_bytes(const cp_pose_targets_track_det_desc* d) {
    if (!d || !cp_pose_targets_track_ws_bytes(&d->track)) return 0;
    Carve c{nullptr};
    ptkd_carve(c, d);
    return c.off;
}

int cp_launch_pose_targets_track_det(hipStream_t s, const cp_pose_targets_track_det_desc* d, void* ws) {
    Carve c{(char*)ws};
    const DetWs w = ptkd_carve(c, d);
    const cp_pose_targets_track_desc* t = &d->track;
    const size_t B = t->cur.B;
    cp_ptk_ws_view v;
    if (cp_ptk_stage(s, t, w.track, &v) != CP_OK ||
        hipMemcpyAsync(w.gen, d->gen, B * CP_PTKD_GEN_STRIDE * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
        return CP_ERR_LAUNCH;
    bool any = false;  // a batch without a mode-1 image skips the matching
    for (size_t b = 0; b < B; ++b) any = any || d->gen[b * CP_PTKD_GEN_STRIDE + CP_PTKD_GEN_MODE] != 0.0;
    if (any)
        hipLaunchKernelGGL(det_boxes_match_kernel, dim3((unsigned)B), dim3(64), 0, s, t->max_pre_objs, d->K_det, d->cat_rule,
                           v.img, v.timg, v.pre, (const double*)w.gen, d->det_post, d->det_count, d->det_pnp, w.match);
    PtkDetOpts dop;
    dop.render_hm_mode = d->render_hm_mode, dop.render_hmhp_mode = d->render_hmhp_mode, dop.cat_rule = d->cat_rule;
    hipLaunchKernelGGL(pre_objects_det_kernel, dim3((unsigned)B), dim3(64), 0, s, cp_ptk_opts(t), dop, t->cur.S, t->max_pre_objs,
                       v.img, v.timg, v.pre, (const double*)w.gen, (const double*)w.match, (PtkPreOut*)v.res, v.counts,
                       (int4*)v.draws, v.peaks);
    return cp_ptk_finish(s, t, w.track);
}
