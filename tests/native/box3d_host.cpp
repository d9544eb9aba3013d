// Host build of centerpose_amd/csrc/box3d_common.h for tests/test_box_metrics_cpu.py: the same source box3d.hip's
// box_iou_kernel and box_eval_kernel run, one pair after the other, rotation indices in ascending order (the reduction
// the kernel does across lanes is the sequential scan here).
#include "../../centerpose_amd/csrc/box3d_common.h"

using namespace box3d;

extern "C" void box_host_iou(const double* a, const double* b, int n, double* iou, int* flags) {
    double bufA[MAXV * 3], bufB[MAXV * 3];
    for (int i = 0; i < n; ++i) {
        int f = 0;
        iou[i] = box_iou(a + i * 27, b + i * 27, bufA, bufB, 1, f);
        flags[i] = f;
    }
}

extern "C" void box_host_eval(const double* pred3d, const double* gt3d, const double* pred2d, const double* mo2c,
                              const double* proj, const int* single, int n, int num_symmetry, double* out) {
    double bufA[MAXV * 3], bufB[MAXV * 3];
    for (int p = 0; p < n; ++p) {
        const double *pr = pred3d + p * 27, *gt = gt3d + p * 27, *p2 = pred2d + p * 18;
        const int nr = single[p] ? 1 : num_symmetry;
        double mc2o[16];
        const bool ok = inv4(mo2c + p * 16, mc2o);
        Best3 b3 = {0., 0., 0., 0., 0., -1, 0};
        Best2 b2 = {0., -1};
        int clip = 0;
        for (int r = 0; r < nr; ++r) {
            eval_rotation3(pr, gt, r, num_symmetry, bufA, bufB, 1, b3, clip);
            if (ok) eval_rotation2(p2, gt, proj + p * 16, mo2c + p * 16, mc2o, r, num_symmetry, b2);
        }
        write_record(pr, gt, num_symmetry, b3, b2, clip, ok, out + p * CP_BOX_EVAL_STRIDE);
    }
}

extern "C" void box_host_fit(const double* v, double* R, double* t, double* s) {
    Fit f;
    box_fit(v, f);
    for (int k = 0; k < 9; ++k) R[k] = f.R[k];
    for (int k = 0; k < 3; ++k) t[k] = f.t[k], s[k] = f.s[k];
}

extern "C" int box_host_inside(const double* v, const double* p) {
    Fit f;
    box_fit(v, f);
    return box_inside(f, p) ? 1 : 0;
}

extern "C" void box_host_rotate(const double* v, double theta, double* out) { rotate_box(v, theta, out); }

extern "C" double box_host_volume(const double* v) { return box_volume(v); }

// one Sutherland-Hodgman pass (clip_poly) on a host polygon: in [n][3] -> out [MAXV][3], returns the vertex count
extern "C" int box_host_clip(const double* in, int n, double plane, double normal, int axis, double* out, int* flags) {
    double a[MAXV * 3];
    for (int k = 0; k < n * 3 && k < MAXV * 3; ++k) a[k] = in[k];
    int f = 0;
    const int m = clip_poly(a, n, out, 1, plane, normal, axis, f);
    *flags = f;
    return m;
}
