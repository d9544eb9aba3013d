// Host build of centerpose_amd/csrc/pose_targets_track_common.h for tests/test_pose_targets_track_cpu.py: the
// previous-frame objects kernel's per-object logic, evaluated on the host and flattened for ctypes.
#include "../../centerpose_amd/csrc/pose_targets_track_common.h"

using namespace pose_targets;

// opts[15]: input_w, input_h, down_ratio, center_3D, pre_hm, pre_hm_hp, hm_heat_random, hm_hp_heat_random,
//           tracking_label_mode, hm_disturb, lost_disturb, fp_disturb, hm_hp_disturb, hp_lost_disturb, hp_fp_disturb
// out[103]: kept, id, chosen, cts_none, cts (2), pts (16), pmask (8), radius, then per channel (9) and draw (own, false
//           positive): on, x, y, k
extern "C" void ptk_host_pre_object(const double* img, const double* pre, int S, const double* opts, double* out) {
    PtkOpts op;
    op.input_w = (int)opts[0], op.input_h = (int)opts[1], op.down_ratio = (int)opts[2];
    op.center_3D = (int)opts[3], op.pre_hm = (int)opts[4], op.pre_hm_hp = (int)opts[5];
    op.hm_heat_random = (int)opts[6], op.hm_hp_heat_random = (int)opts[7], op.tracking_label_mode = (int)opts[8];
    op.hm_disturb = opts[9], op.lost_disturb = opts[10], op.fp_disturb = opts[11];
    op.hm_hp_disturb = opts[12], op.hp_lost_disturb = opts[13], op.hp_fp_disturb = opts[14];
    PtkPre r;
    ptk_pre_object(img, pre, S, op, &r);
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
