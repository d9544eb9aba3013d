// Host build of centerpose_amd/csrc/pose_targets_common.h for tests/test_pose_targets_cpu.py: the objects kernel's
// per-(object, variant) logic, evaluated on the host and flattened for ctypes.
#include "../../centerpose_amd/csrc/pose_targets_common.h"

using namespace pose_targets;

// out[52]: kept, radius, ct (2), ind, wh (2), reg (2), scale (3), joint_ok (8), pt (8 x 2), hps (16)
extern "C" void pt_host_object(const double* img, const double* obj, int s, int S, int R, int flags, double* out) {
    PtResult r;
    pt_object(img, obj, s, S, R, flags, &r);
    for (int i = 0; i < 52; ++i) out[i] = 0.0;
    out[0] = r.kept;
    if (!r.kept) return;
    out[1] = r.radius;
    out[2] = r.ct[0], out[3] = r.ct[1];
    out[4] = (double)r.ind;
    out[5] = r.wh[0], out[6] = r.wh[1], out[7] = r.reg[0], out[8] = r.reg[1];
    for (int i = 0; i < 3; ++i) out[9 + i] = r.scale[i];
    for (int j = 0; j < CP_PT_JOINTS; ++j) {
        out[12 + j] = r.joint_ok[j];
        out[20 + 2 * j] = r.pt[j][0], out[21 + 2 * j] = r.pt[j][1];
        out[36 + 2 * j] = r.hps[2 * j], out[37 + 2 * j] = r.hps[2 * j + 1];
    }
}
