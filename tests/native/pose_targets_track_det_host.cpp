// Host build of centerpose_amd/csrc/pose_targets_track_det_common.h for tests/test_pose_targets_track_det_cpu.py: the
// matching of a detector's boxes to one image's previous objects and the detector-fed per-object logic, evaluated on
// the host and flattened for ctypes.
#include "../../centerpose_amd/csrc/pose_targets_track_det_common.h"

using namespace pose_targets;

// match [npre][64]: the records det_boxes_match_kernel leaves (PTKD_* layout)
extern "C" void ptkd_host_match(const double* img, const double* pre, int npre, int cat_rule, const double* post,
                                const double* pnp, int count, int K_det, double* match) {
    ptkd_match_image(img, pre, npre, cat_rule, post, pnp, count, K_det, match);
}

// opts[15] and out[103] as ptk_host_pre_object's (pose_targets_track_host.cpp); dopts[3]: render_hm_mode,
// render_hmhp_mode, cat_rule; m: the object's match record
extern "C" void ptkd_host_pre_object(const double* img, const double* pre, const double* m, double radius_scale, int S,
                                     const double* opts, const int* dopts, double* out) {
    PtkOpts op;
    op.input_w = (int)opts[0], op.input_h = (int)opts[1], op.down_ratio = (int)opts[2];
    op.center_3D = (int)opts[3], op.pre_hm = (int)opts[4], op.pre_hm_hp = (int)opts[5];
    op.hm_heat_random = (int)opts[6], op.hm_hp_heat_random = (int)opts[7], op.tracking_label_mode = (int)opts[8];
    op.hm_disturb = opts[9], op.lost_disturb = opts[10], op.fp_disturb = opts[11];
    op.hm_hp_disturb = opts[12], op.hp_lost_disturb = opts[13], op.hp_fp_disturb = opts[14];
    PtkDetOpts dop;
    dop.render_hm_mode = dopts[0], dop.render_hmhp_mode = dopts[1], dop.cat_rule = dopts[2];
    PtkPre r;
    ptk_pre_object_det(img, pre, m, radius_scale, S, op, dop, &r);
    for (int i = 0; i < 103; ++i) out[i] = 0.0;
    out[0] = r.o.kept, out[1] = r.o.id, out[2] = r.o.chosen, out[3] = r.o.cts_none;
    out[4] = r.o.cts[0], out[5] = r.o.cts[1];
    for (int i = 0; i < 2 * CP_PT_JOINTS; ++i) out[6 + i] = r.o.pts[i];
    for (int j = 0; j < CP_PT_JOINTS; ++j) out[22 + j] = (r.o.pmask >> j) & 1u;
    out[30] = r.radius;
    for (int c = 0; c < 1 + CP_PT_JOINTS; ++c)
        for (int f = 0; f < 2; ++f) {
            double* o = out + 31 + 4 * (2 * c + f);
            o[0] = r.draw_on[c][f];
            if (!r.draw_on[c][f]) continue;
            o[1] = r.draw_xy[c][f][0], o[2] = r.draw_xy[c][f][1], o[3] = r.draw_k[c][f];
        }
}
