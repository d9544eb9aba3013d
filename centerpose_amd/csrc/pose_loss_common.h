// Per-element formulas of ObjectPoseLoss (pose_loss.hip) and their derivatives, written so that the host compiler can
// build them too (tests/native/pose_loss_host.cpp; tests/test_pose_loss_cpu.py pins them to the float64 restatement
// tests/pose_loss_ref.py).  Each routine restates one expression of the reference:
//   pl_clamp / pl_sigmoid          models/utils.py:9-11   clamp(x.sigmoid_(), 1e-4, 1 - 1e-4)
//   pl_focal_pos / pl_focal_neg    models/losses.py:61-63 log(p) (1-p)^2 [gt == 1],  log(1-p) p^2 (1-gt)^4 [gt < 1]
//   pl_focal_dlogit                d/dlogit of coef * (focal term of gt): the clamp passes the gradient where
//                                  1e-4 <= y <= 1-1e-4 (torch's clamp backward, inclusive), sigmoid's is y (1 - y)
//   pl_reg_value / pl_reg_grad     models/losses.py:143-226, :243-254, one gathered element of RegL1Loss (plain, residual,
//                                  relative), RegWeightedL1Loss (= plain with an element mask), RegKLDKeyLoss, RegKLDScaleLoss
// abs' derivative is sgn(x), 0 at 0, as torch's.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define PL_HD __host__ __device__ inline
#else
#define PL_HD inline
#endif

namespace pose_loss {

using std::exp;
using std::fabs;
using std::log;

enum RegMode : int {
    PL_L1 = 0,         // |t*m - p*m|                                 (RegL1Loss, RegWeightedL1Loss)
    PL_L1_RESID = 1,   // |t*m - q*m|, q = exp(p) * ref               (RegL1Loss with dimension_ref, use_residual)
    PL_L1_REL = 2,     // |(1*m - p*m) / t'|, t' = t or 1e-6 where 0  (RegL1Loss relative_loss, val phase)
    PL_KLD_KEY = 3,    // a = (t*m - p*m)^2                           (RegKLDKeyLoss)
    PL_KLD_SCALE = 4,  // a = (t - p)^2 * m                           (RegKLDScaleLoss)
};

// denominators: sum(mask) + eps
PL_HD float reg_eps(int mode) { return mode >= PL_KLD_KEY ? 1e-6f : 1e-4f; }

template <class T>
PL_HD T lo_bound() { return (T)(float)1e-4; }
template <class T>
PL_HD T hi_bound() { return (T)(float)(1.0 - 1e-4); }

template <class T>
PL_HD T pl_sigmoid(T x) { return (T)1 / ((T)1 + exp(-x)); }

template <class T>
PL_HD T pl_clamp(T y) { return y < lo_bound<T>() ? lo_bound<T>() : (y > hi_bound<T>() ? hi_bound<T>() : y); }

template <class T>
PL_HD T pl_sgn(T x) { return x > (T)0 ? (T)1 : (x < (T)0 ? (T)-1 : (T)0); }

template <class T>
PL_HD T pl_focal_pos(T p) { return log(p) * ((T)1 - p) * ((T)1 - p); }

template <class T>
PL_HD T pl_focal_negw(T g) {
    const T w = (T)1 - g;
    return w * w * w * w;
}

template <class T>
PL_HD T pl_focal_neg(T p) { return log((T)1 - p) * p * p; }

// d/dp of the focal term of one element with ground truth g (0 where g > 1 or NaN: neither predicate holds)
template <class T>
PL_HD T pl_focal_dp(T p, T g) {
    if (g == (T)1) return ((T)1 - p) * ((T)1 - p) / p - (T)2 * ((T)1 - p) * log(p);
    if (g < (T)1) return pl_focal_negw(g) * ((T)2 * p * log((T)1 - p) - p * p / ((T)1 - p));
    return (T)0;
}

// coef * d(focal term)/dlogit given the in-place sigmoid y
template <class T>
PL_HD T pl_focal_dlogit(T y, T g, T coef) {
    if (!(y >= lo_bound<T>() && y <= hi_bound<T>())) return (T)0;
    return coef * pl_focal_dp(y, g) * (y * ((T)1 - y));
}

// One gathered element: t target, p prediction, m mask, u uncertainty (KLD), ref dimension_ref (residual), kl the KL scale.
template <class T>
PL_HD T pl_reg_value(int mode, T t, T p, T m, T u, T ref, T kl) {
    switch (mode) {
        case PL_L1: return fabs(t * m - p * m);
        case PL_L1_RESID: {
            const T q = exp(p) * ref;
            return fabs(t * m - q * m);
        }
        case PL_L1_REL: {
            const T tr = t == (T)0 ? (T)1e-6f : t;
            return fabs(((T)1 * m - p * m) / tr);
        }
        default: {
            const T d = mode == PL_KLD_KEY ? t * m - p * m : t - p;
            const T a = mode == PL_KLD_KEY ? d * d : d * d * m;
            const T v = exp(u);
            return (u - log(kl) + (kl * exp(-a / kl) + a) / v - (T)1 + (T)0.5 * fabs(v)) * m;
        }
    }
}

// d value / dp -> *dp, d value / du -> *du (0 for the L1 modes)
template <class T>
PL_HD void pl_reg_grad(int mode, T t, T p, T m, T u, T ref, T kl, T* dp, T* du) {
    *du = (T)0;
    switch (mode) {
        case PL_L1: *dp = -m * pl_sgn(t * m - p * m); return;
        case PL_L1_RESID: {
            const T q = exp(p) * ref;
            *dp = -m * pl_sgn(t * m - q * m) * q;
            return;
        }
        case PL_L1_REL: {
            const T tr = t == (T)0 ? (T)1e-6f : t;
            *dp = pl_sgn(((T)1 * m - p * m) / tr) * (-m / tr);
            return;
        }
        default: {
            const T d = mode == PL_KLD_KEY ? t * m - p * m : t - p;
            const T a = mode == PL_KLD_KEY ? d * d : d * d * m;
            const T v = exp(u);
            const T e = exp(-a / kl);
            const T dvda = m * ((T)1 - e) / v;
            *dp = dvda * ((T)-2 * d * m);  // both forms: da/dp = -2 d m
            *du = m * ((T)1 - (kl * e + a) / v + (T)0.5 * v);
            return;
        }
    }
}

}  // namespace pose_loss
