// Host build of centerpose_amd/csrc/pose_loss_common.h for tests/test_pose_loss_cpu.py: the per-element formulas and
// derivatives pose_loss.hip runs, evaluated element by element in float64 (and float32, the device's type).
#include "../../centerpose_amd/csrc/pose_loss_common.h"

using namespace pose_loss;

template <class T>
static void focal(int n, const double* x, const double* g, double* p, double* pos, double* neg, double* dlogit) {
    for (int i = 0; i < n; ++i) {
        const T y = pl_sigmoid((T)x[i]), q = pl_clamp(y);
        p[i] = (double)q;
        pos[i] = (double)pl_focal_pos(q);
        neg[i] = (double)(pl_focal_neg(q) * pl_focal_negw((T)g[i]));
        dlogit[i] = (double)pl_focal_dlogit(y, (T)g[i], (T)1);
    }
}

template <class T>
static void reg(int mode, int n, const double* t, const double* p, const double* m, const double* u, double ref,
                double kl, double* val, double* dp, double* du) {
    for (int i = 0; i < n; ++i) {
        T a, b;
        val[i] = (double)pl_reg_value<T>(mode, (T)t[i], (T)p[i], (T)m[i], (T)u[i], (T)ref, (T)kl);
        pl_reg_grad<T>(mode, (T)t[i], (T)p[i], (T)m[i], (T)u[i], (T)ref, (T)kl, &a, &b);
        dp[i] = (double)a, du[i] = (double)b;
    }
}

extern "C" void pl_host_focal(int f32, int n, const double* x, const double* g, double* p, double* pos, double* neg,
                              double* dlogit) {
    if (f32) focal<float>(n, x, g, p, pos, neg, dlogit);
    else focal<double>(n, x, g, p, pos, neg, dlogit);
}

extern "C" void pl_host_reg(int f32, int mode, int n, const double* t, const double* p, const double* m, const double* u,
                            double ref, double kl, double* val, double* dp, double* du) {
    if (f32) reg<float>(mode, n, t, p, m, u, ref, kl, val, dp, du);
    else reg<double>(mode, n, t, p, m, u, ref, kl, val, dp, du);
}
