// The per-pixel arithmetic of train_inputs.hip: one output pixel of ObjectPoseDataset._get_input
// (datasets/dataset_combined.py:278-288) with color_aug (utils/image.py:239-277), written so that the host compiler can
// build it too (tests/native/train_inputs_host.cpp, tests/test_train_inputs_cpu.py pins it to the numpy restatement
// tests/train_inputs_ref.py).  Steps, as include/centerpose_hip.h numbers them: 1 ti_warp, 2 ti_scale, 3 ti_grey /
// ti_color, 4 ti_normalise.
#pragma once
#include <math.h>

// record layout of include/centerpose_hip.h (float64), repeated here so that the host build needs no HIP header; an
// identical redefinition is legal, a drifting one is a compile error
#define CP_TI_STRIDE 24
#define CP_TI_OFFSET 0
#define CP_TI_HEIGHT 1
#define CP_TI_WIDTH 2
#define CP_TI_TRANS 3
#define CP_TI_FLIPPED 9
#define CP_TI_COLOR 10
#define CP_TI_ORDER 11
#define CP_TI_ALPHA 12
#define CP_TI_SHIFT 15

// No fused multiply-adds in either build: every operation below restates a numpy operation that rounds on its own
// (hipcc's default, -ffp-contract=fast, would fuse the blends' products into their sums).  Restored at the end.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
#ifdef __HIPCC__
#define TI_HD __host__ __device__ __forceinline__
#else
#define TI_HD static inline
#endif

namespace train_inputs {

// the three colour operations and the 6 orders random.shuffle can leave them in (CP_TI_ORDER)
constexpr int TI_BRIGHTNESS = 0, TI_CONTRAST = 1, TI_SATURATION = 2;
TI_HD int ti_order_op(int order, int i) {
    // six bits per order, two per operation, first run in the low bits: bcs, bsc, cbs, csb, sbc, scb
    const unsigned long long table = (0ull | 1 << 2 | 2 << 4) | (0ull | 2 << 2 | 1 << 4) << 6 | (1ull | 0 << 2 | 2 << 4) << 12 |
                                     (1ull | 2 << 2 | 0 << 4) << 18 | (2ull | 0 << 2 | 1 << 4) << 24 | (2ull | 1 << 2 | 0 << 4) << 30;
    return (int)((table >> (6 * order + 2 * i)) & 3);
}

// one image's record, decoded once (per workgroup on the device)
struct TiImage {
    long long offset;  // of the frame in the frames buffer, bytes
    int H, W, flipped, color, order;
    double m[6];      // INVERSE map (destination -> source), float64 as cv::invertAffineTransform leaves it
    float a[3], b[3];  // per operation run: float32(alpha), float32(1.0 - alpha)
    double shift[3];   // lighting, per B, G, R
};

// cv::invertAffineTransform (float64), as cp_launch_preprocess: warpAffine without WARP_INVERSE_MAP inverts the forward
// matrix first; a singular matrix gives the zero matrix
TI_HD void ti_invert(const double* M, double* m) {
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1.0 / D : 0.0;
    const double A11 = M[4] * D, A22 = M[0] * D, A12 = -M[1] * D, A21 = -M[3] * D;
    m[0] = A11, m[1] = A12, m[2] = -A11 * M[2] - A12 * M[5];
    m[3] = A21, m[4] = A22, m[5] = -A21 * M[2] - A22 * M[5];
}

TI_HD void ti_decode(const double* rec, TiImage* im) {
    im->offset = (long long)rec[CP_TI_OFFSET];
    im->H = (int)rec[CP_TI_HEIGHT], im->W = (int)rec[CP_TI_WIDTH];
    im->flipped = rec[CP_TI_FLIPPED] != 0.0, im->color = rec[CP_TI_COLOR] != 0.0;
    im->order = (int)rec[CP_TI_ORDER];
    ti_invert(rec + CP_TI_TRANS, im->m);
    for (int i = 0; i < 3; ++i) {
        // `1. + data_rng.uniform(...)` is a Python float: numpy rounds it to float32 for `image *= alpha`, and rounds
        // the Python float `1 - alpha` to float32 for `image2 *= (1 - alpha)`
        im->a[i] = (float)rec[CP_TI_ALPHA + i];
        im->b[i] = (float)(1.0 - rec[CP_TI_ALPHA + i]);
        im->shift[i] = rec[CP_TI_SHIFT + i];
    }
}

// Step 1: the 8-bit levels of cv2.warpAffine(INTER_LINEAR, constant 0 border) at destination (x, y), OpenCV's fixed-point
// arithmetic as preprocess_kernel (ewise.hip) and oracle/cv_emul.py state it.  `img` is the frame's first byte; a tap is
// read only inside [0, W) x [0, H), so nothing outside the frame's 3 H W bytes is touched whatever the matrix holds.
// rint() = lrint / cvRound: round half to even.  The clamp at +-2^52 (a NaN goes to -2^52) changes no coordinate an image
// of fewer than 2^31 columns can hold; it keeps the conversion and the sums below defined for a near-singular matrix.
TI_HD long long ti_fix(double v) {
    const double lim = 4503599627370496.0;
    if (!(v > -lim)) v = -lim;
    if (v > lim) v = lim;
    return (long long)rint(v);
}

TI_HD void ti_warp(const unsigned char* img, int H, int W, int flipped, const double* m, int x, int y, int* v8) {
    const long long adelta = ti_fix(m[0] * (double)x * 1024.0), bdelta = ti_fix(m[3] * (double)x * 1024.0);
    const long long X0 = ti_fix((m[1] * (double)y + m[2]) * 1024.0) + 16;
    const long long Y0 = ti_fix((m[4] * (double)y + m[5]) * 1024.0) + 16;
    const long long X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
    const long long sx = X >> 5, sy = Y >> 5;
    const int fx = (int)(X & 31), fy = (int)(Y & 31);
    int acc[3] = {0, 0, 0};
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const long long xx = sx + dx, yy = sy + dy;
            if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
            const int wgt = (dx ? fx : 32 - fx) * (dy ? fy : 32 - fy) * 32;
            // the reference warps img[:, ::-1, :]: column xx of the flipped view is column W - 1 - xx of the frame
            const long long col = flipped ? (long long)W - 1 - xx : xx;
            const unsigned char* px = img + ((size_t)yy * (size_t)W + (size_t)col) * 3;
            acc[0] += wgt * px[0];
            acc[1] += wgt * px[1];
            acc[2] += wgt * px[2];
        }
    for (int c = 0; c < 3; ++c) v8[c] = (acc[c] + (1 << 14)) >> 15;
}

// Step 2: inp.astype(np.float32) / 255., a float32 division
TI_HD float ti_scale(int v8) { return (float)v8 / 255.f; }

// Step 3, BGR2GRAY of a float image
TI_HD float ti_grey(const float* v) { return (0.114f * v[0] + 0.587f * v[1]) + 0.299f * v[2]; }

// Step 3: the three operations in the record's order, then lighting.  gs and gs_mean are those of the image before any
// operation (blend_ scales the reference's gs in place, but saturation_ is its only reader)
TI_HD void ti_color(float* v, float gs, float gs_mean, const TiImage* im) {
    for (int i = 0; i < 3; ++i) {
        const int op = ti_order_op(im->order, i);
        const float a = im->a[i], b = im->b[i];
        if (op == TI_BRIGHTNESS) {
            for (int c = 0; c < 3; ++c) v[c] = v[c] * a;
        } else {
            const float t = (op == TI_CONTRAST ? gs_mean : gs) * b;
            for (int c = 0; c < 3; ++c) v[c] = v[c] * a + t;
        }
    }
    for (int c = 0; c < 3; ++c) v[c] = (float)((double)v[c] + im->shift[c]);  // a float64 array into the float32 image
}

// Step 4: (inp - mean) / std with float32 mean / std
TI_HD float ti_normalise(float v, float mean, float std) { return (v - mean) / std; }

// steps 1 + 2 of one pixel, and its grey value
TI_HD float ti_pixel(const unsigned char* img, const TiImage* im, int x, int y, float* v) {
    int v8[3];
    ti_warp(img, im->H, im->W, im->flipped, im->m, x, y, v8);
    for (int c = 0; c < 3; ++c) v[c] = ti_scale(v8[c]);
    return ti_grey(v);
}

}  // namespace train_inputs

#if defined(__clang__)
#pragma clang fp contract(fast)  // hipcc's default again for whatever the including file defines after this header
#endif
