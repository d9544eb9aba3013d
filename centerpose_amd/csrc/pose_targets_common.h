// The scalar logic of pose_targets.hip's objects kernel: the training targets of ONE object in ONE symmetry variant, as
// ObjectPoseDataset.__getitem__ builds them for the current frame (datasets/dataset_combined.py:957-1130), written so
// that the host compiler can build it too (tests/native/pose_targets_host.cpp, tests/test_pose_targets_cpu.py pins it to
// the float64 restatement tests/pose_targets_ref.py).
#pragma once
#include <math.h>

// record layouts of include/centerpose_hip.h (float64), repeated here so that the host build needs no HIP header; an
// identical redefinition is legal, a drifting one is a compile error
#define CP_PT_IMG_STRIDE 32
#define CP_PT_IMG_TRANS 0
#define CP_PT_IMG_WIDTH 6
#define CP_PT_IMG_HEIGHT 7
#define CP_PT_IMG_FLIPPED 8
#define CP_PT_IMG_ROT 9
#define CP_PT_IMG_NUM_OBJS 10
#define CP_PT_IMG_PROJ 11
#define CP_PT_OBJ_STRIDE 64
#define CP_PT_OBJ_NSYM 0
#define CP_PT_OBJ_CUBOID 1
#define CP_PT_OBJ_QUAT 19
#define CP_PT_OBJ_LOC 23
#define CP_PT_OBJ_KPS3D 26
#define CP_PT_OBJ_SCALE 53
#define CP_PT_JOINTS 8

// No fused multiply-adds in either build: every operation below restates a numpy / Python float64 operation that rounds
// on its own (hipcc's default, -ffp-contract=fast, would fuse e.g. the affine's products into its sums, and a truncation
// to int would then differ from the host build's).  Restored at the end of the header.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
#ifdef __HIPCC__
#define PT_HD __host__ __device__ __forceinline__
#else
#define PT_HD static inline
#endif

namespace pose_targets {

// flags of pt_object (cp_pose_targets_desc's options)
constexpr int PT_CENTER_3D = 1;
constexpr int PT_ABS_SCALE = 2;

// what one (object, variant) contributes; kept == 0: nothing (every sparse slot of it stays 0, no draw)
struct PtResult {
    int kept;            // reg_mask
    int radius;          // the centre's and the joints' Gaussian radius (hp_radius = radius, :1086)
    int ct[2];           // ct_int (x, y): the centre draw
    long long ind;       // ct_int[1] * R + ct_int[0]
    float wh[2], reg[2], scale[3];
    int joint_ok[CP_PT_JOINTS];  // hps_mask / hp_mask set and a hm_hp draw at pt[j]
    int pt[CP_PT_JOINTS][2];     // pt_int (x, y)
    float hps[2 * CP_PT_JOINTS];
};

// int(v) / an assignment into int64: truncation toward zero (the clamp only keeps the conversion defined for points far
// behind the camera, whose coordinates are out of every test below anyway)
PT_HD long long pt_trunc(double v) {
    if (!(v < 4.0e18)) return v != v ? 0 : 4000000000000000000LL;
    if (!(v > -4.0e18)) return -4000000000000000000LL;
    return (long long)v;
}

// affine_transform (utils/image.py:71-74): the point goes through float32, the product with the float64 2x3 is float64.
// np.dot evaluates each 3-term row in BLAS as fma(t0, x, t1 * y) + t2 (bit-identical to numpy's result on every row of
// the reference-built goldens); the order matters where a box edge lands next to an integer and ceil() reads it.
PT_HD void pt_affine(const double* t, double x, double y, double* ox, double* oy) {
    const double fx = (double)(float)x, fy = (double)(float)y;
    *ox = fma(t[0], fx, t[1] * fy) + t[2];
    *oy = fma(t[3], fx, t[4] * fy) + t[5];
}

PT_HD void pt_mat4(const double* a, const double* b, double* c) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = a[i * 4] * b[j];
            for (int k = 1; k < 4; ++k) s = s + a[i * 4 + k] * b[k * 4 + j];
            c[i * 4 + j] = s;
        }
}

// the variant projection (:982-1010): P . M_o2c . rotation_y(theta * s) . M_o2c^-1, homogeneous divide, viewport, and
// int() of each coordinate; out[i] = (int(vp[1]), int(vp[0])) for the 9 keypoints (centre first)
PT_HD void pt_project(const double* img, const double* obj, int s, int S, long long out[9][2]) {
    const double* q = obj + CP_PT_OBJ_QUAT;  // Rotation.from_quat(xyzw).as_matrix(), q normalised first
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double x = q[0] / n, y = q[1] / n, z = q[2] / n, w = q[3] / n;
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    const double r[9] = {x2 - y2 - z2 + w2, 2 * (xy - zw),      2 * (xz + yw),
                         2 * (xy + zw),     -x2 + y2 - z2 + w2, 2 * (yz - xw),
                         2 * (xz - yw),     2 * (yz + xw),      -x2 - y2 + z2 + w2};
    const double* t = obj + CP_PT_OBJ_LOC;
    double o2c[16], c2o[16], ry[16], m0[16], m1[16], m[16];
    for (int i = 0; i < 3; ++i) {  // M_o2c and its rigid inverse [R^T, -R^T t]
        for (int j = 0; j < 3; ++j) {
            o2c[i * 4 + j] = r[i * 3 + j];
            c2o[i * 4 + j] = r[j * 3 + i];
        }
        o2c[i * 4 + 3] = t[i];
        c2o[i * 4 + 3] = -(r[i] * t[0] + r[3 + i] * t[1] + r[6 + i] * t[2]);
        o2c[12 + i] = c2o[12 + i] = 0.0;
    }
    o2c[15] = c2o[15] = 1.0;
    const double theta = 2 * M_PI / S, a = theta * s, cs = cos(a), sn = sin(a);  // rotation_y_matrix (:33-37)
    const double ryv[16] = {cs, 0, sn, 0, 0, 1, 0, 0, -sn, 0, cs, 0, 0, 0, 0, 1};
    for (int i = 0; i < 16; ++i) ry[i] = ryv[i];
    pt_mat4(img + CP_PT_IMG_PROJ, o2c, m0);
    pt_mat4(m0, ry, m1);
    pt_mat4(m1, c2o, m);
    const double width = img[CP_PT_IMG_WIDTH], height = img[CP_PT_IMG_HEIGHT];
    for (int i = 0; i < 9; ++i) {
        const double* k = obj + CP_PT_OBJ_KPS3D + 3 * i;
        double p[4];
        for (int row = 0; row < 4; ++row)
            p[row] = m[row * 4] * k[0] + m[row * 4 + 1] * k[1] + m[row * 4 + 2] * k[2] + m[row * 4 + 3] * 1.0;
        const double v0 = (p[0] / p[3] + 1.0) / 2.0 * height, v1 = (p[1] / p[3] + 1.0) / 2.0 * width;
        out[i][0] = pt_trunc(v1);
        out[i][1] = pt_trunc(v0);
    }
}

// gaussian_radius (utils/image.py:103-123) of (ceil h, ceil w), with its (b + sq) / 2; the caller takes max(0, int(.))
PT_HD double pt_gaussian_radius(double height, double width) {
    const double mo = 0.7;
    const double b1 = height + width;
    const double c1 = width * height * (1 - mo) / (1 + mo);
    const double r1 = (b1 + sqrt(b1 * b1 - 4 * c1)) / 2;
    const double b2 = 2 * (height + width);
    const double c2 = (1 - mo) * width * height;
    const double r2 = (b2 + sqrt(b2 * b2 - 16 * c2)) / 2;
    const double a3 = 4 * mo;
    const double b3 = -2 * mo * (height + width);
    const double c3 = (mo - 1) * width * height;
    const double r3 = (b3 + sqrt(b3 * b3 - 4 * a3 * c3)) / 2;
    double r = r1;
    if (r2 < r) r = r2;
    if (r3 < r) r = r3;
    return r;
}

// one object k of one image in variant s (s < the object's variant count); R = output_res
PT_HD void pt_object(const double* img, const double* obj, int s, int S, int R, int flags, PtResult* res) {
    res->kept = 0;
    const double* tr = img + CP_PT_IMG_TRANS;
    const double width = img[CP_PT_IMG_WIDTH], height = img[CP_PT_IMG_HEIGHT];
    const bool flipped = img[CP_PT_IMG_FLIPPED] != 0.0;
    // the 9 points: float64 projected_cuboid, or the variant's re-projected integers (variant 0 included, :980)
    double p[9][2];
    long long pi[8][2];
    if ((int)obj[CP_PT_OBJ_NSYM] != 1) {
        long long q[9][2];
        pt_project(img, obj, s, S, q);
        for (int i = 0; i < 9; ++i) p[i][0] = (double)q[i][0], p[i][1] = (double)q[i][1];
    } else {
        for (int i = 0; i < 9; ++i) p[i][0] = obj[CP_PT_OBJ_CUBOID + 2 * i], p[i][1] = obj[CP_PT_OBJ_CUBOID + 2 * i + 1];
    }
    // visibility on the unrounded corner, the stored corner truncated into int64 (:1015-1020)
    int vis[8], vsum = 0;
    for (int i = 0; i < 8; ++i) {
        const double x = p[i + 1][0], y = p[i + 1][1];
        vis[i] = (x >= width || x < 0 || y < 0 || y >= height) ? 1 : 2;
        vsum += vis[i];
        pi[i][0] = pt_trunc(x);
        pi[i][1] = pt_trunc(y);
    }
    if (flipped) {  // :1023-1028, flip_idx [[1,5],[3,7],[2,6],[4,8]] on the 8 corners
        const long long wi = (long long)width;
        for (int i = 0; i < 8; ++i) pi[i][0] = wi - pi[i][0] - 1;
        const int sw[4][2] = {{0, 4}, {2, 6}, {1, 5}, {3, 7}};
        for (int e = 0; e < 4; ++e) {
            const int a = sw[e][0], b = sw[e][1];
            for (int c = 0; c < 2; ++c) {
                const long long tmp = pi[a][c];
                pi[a][c] = pi[b][c];
                pi[b][c] = tmp;
            }
            const int tv = vis[a];
            vis[a] = vis[b];
            vis[b] = tv;
        }
    }
    // bounding_box_rotation, then np.clip(., 0, R-1) (:1030-1033)
    double bb[4];
    for (int i = 0; i < 8; ++i) {
        double x, y;
        pt_affine(tr, (double)pi[i][0], (double)pi[i][1], &x, &y);
        if (i == 0 || x < bb[0]) bb[0] = x;
        if (i == 0 || y < bb[1]) bb[1] = y;
        if (i == 0 || x > bb[2]) bb[2] = x;
        if (i == 0 || y > bb[3]) bb[3] = y;
    }
    const double hi = (double)(R - 1);
    for (int i = 0; i < 4; ++i) bb[i] = bb[i] < 0.0 ? 0.0 : (bb[i] > hi ? hi : bb[i]);
    const double h = bb[3] - bb[1], w = bb[2] - bb[0];
    // most corners out of frame and the centre too: dropped (:1036-1039)
    const double cx0 = p[0][0], cy0 = p[0][1];
    const bool visible = !((cx0 >= width || cx0 < 0 || cy0 < 0 || cy0 >= height) && vsum <= 12);
    if (!(((h > 0 && w > 0) || img[CP_PT_IMG_ROT] != 0.0) && visible)) return;
    const double rr = pt_gaussian_radius(ceil(h), ceil(w));
    const int radius = rr > 0 ? (int)rr : 0;  // max(0, int(radius)); int() truncates toward zero
    double ctx, cty;
    int cix, ciy;
    if (!(flags & PT_CENTER_3D)) {  // bbox midpoint: float64, a float32 array, then int32 (:1045-1048)
        const float fx = (float)((bb[0] + bb[2]) / 2), fy = (float)((bb[1] + bb[3]) / 2);
        ctx = fx, cty = fy;
        cix = (int)fx, ciy = (int)fy;
    } else {  // the affine image of the (flipped) float centre; out of the map: skipped (:1049-1055)
        const double c0 = flipped ? width - cx0 - 1 : cx0;
        pt_affine(tr, c0, cy0, &ctx, &cty);
        const long long lx = pt_trunc(ctx), ly = pt_trunc(cty);
        if (lx >= R || ly >= R || lx < 0 || ly < 0) return;
        cix = (int)lx, ciy = (int)ly;
    }
    res->kept = 1;
    res->radius = radius;
    res->ct[0] = cix, res->ct[1] = ciy;
    res->ind = (long long)ciy * R + cix;
    res->wh[0] = (float)(1. * w), res->wh[1] = (float)(1. * h);
    res->reg[0] = (float)(ctx - (double)cix), res->reg[1] = (float)(cty - (double)ciy);
    const double* sc = obj + CP_PT_OBJ_SCALE;  // |scale| or |scale| / scale[1], signed (:1058-1062)
    for (int i = 0; i < 3; ++i) res->scale[i] = (float)((flags & PT_ABS_SCALE) ? fabs(sc[i]) : fabs(sc[i]) / sc[1]);
    // The reference's num_kpts == 0 branch (:1079-1082) is left out: the flags are 1 or 2, so their sum is at least 8,
    // and its 0.9999 centre value would be covered by the centre's own 1.0 anyway.
    for (int j = 0; j < CP_PT_JOINTS; ++j) {  // :1088-1102: the affine, assigned into int64 (truncation), then the tests
        double x, y;
        pt_affine(tr, (double)pi[j][0], (double)pi[j][1], &x, &y);
        const long long jx = pt_trunc(x), jy = pt_trunc(y);
        const bool ok = vis[j] > 1 && jx >= 0 && jx < R && jy >= 0 && jy < R;
        res->joint_ok[j] = ok;
        res->pt[j][0] = ok ? (int)jx : 0;
        res->pt[j][1] = ok ? (int)jy : 0;
        res->hps[2 * j] = ok ? (float)(jx - cix) : 0.f;
        res->hps[2 * j + 1] = ok ? (float)(jy - ciy) : 0.f;
    }
}

}  // namespace pose_targets

#if defined(__clang__) && defined(__HIPCC__)
#pragma clang fp contract(fast)  // hipcc's default again for whatever the including file defines after this header
#endif
