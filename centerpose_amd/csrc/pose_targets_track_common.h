// The scalar logic of pose_targets_track.hip's previous-frame objects kernel: what ONE object of the previous frame
// contributes to the tracking task's training batch, as ObjectPoseDataset.__getitem__ builds it in its noise-simulation
// mode (datasets/dataset_combined.py:558-937 with data_generation_mode == 0), written so that the host compiler can build
// it too (tests/native/pose_targets_track_host.cpp; tests/test_pose_targets_track_cpu.py pins it to the float64
// restatement tests/pose_targets_track_ref.py).  The structs the two objects kernels exchange are here as well.
#pragma once
#include "pose_targets_common.h"

// record layouts of include/centerpose_hip.h (float64), repeated here so that the host build needs no HIP header; an
// identical redefinition is legal, a drifting one is a compile error
#define CP_PTK_IMG_STRIDE 32
#define CP_PTK_IMG_TRANS 0
#define CP_PTK_IMG_NUM_PRE 6
#define CP_PTK_IMG_PROJ 7
#define CP_PTK_PRE_STRIDE 128
#define CP_PTK_PRE_SKIP 56
#define CP_PTK_PRE_IDSYM 57
#define CP_PTK_PRE_ID 58
#define CP_PTK_PRE_DRAWS 64
#define CP_PTK_DRAW_CT_NOISE 0
#define CP_PTK_DRAW_CT_LOST 2
#define CP_PTK_DRAW_CT_HEAT 3
#define CP_PTK_DRAW_CT_FP 4
#define CP_PTK_DRAW_CT_FP_NOISE 5
#define CP_PTK_DRAW_CT_FP_PEAK 7
#define CP_PTK_DRAW_JOINTS 8
#define CP_PTK_DRAW_JOINT_STRIDE 7
#define CP_PTK_DRAW_J_NOISE 0
#define CP_PTK_DRAW_J_LOST 2
#define CP_PTK_DRAW_J_FP 3
#define CP_PTK_DRAW_J_FP_NOISE 4
#define CP_PTK_DRAW_J_FP_PEAK 6
#define CP_PTK_CUR_STRIDE 2
#define CP_PTK_CUR_ID 0
#define CP_PTK_CUR_SKIP 1

// no fused multiply-adds, as in pose_targets_common.h (which restored hipcc's default at its end)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace pose_targets {

// pow() as numpy's scalar ** calls it.  The host build must not fold pow(x, 2.0) into x * x or pow(2.0, y) into exp2(y):
// libm's pow is not correctly rounded, and the restatement compares the peaks bit for bit.
#ifdef __HIPCC__
PT_HD double ptk_pow(double a, double b) { return pow(a, b); }
#else
static __attribute__((noinline, noclone)) double ptk_pow(double a, double b) {
    volatile double va = a, vb = b;
    return pow(va, vb);
}
#endif

// cp_pose_targets_track_desc's geometry and options
struct PtkOpts {
    int input_w, input_h, down_ratio;
    int center_3D, pre_hm, pre_hm_hp, hm_heat_random, hm_hp_heat_random, tracking_label_mode;
    double hm_disturb, lost_disturb, fp_disturb, hm_hp_disturb, hp_lost_disturb, hp_fp_disturb;
};

// what the previous-frame kernel leaves per previous object for the current-frame kernel
struct PtkPreOut {
    int kept;      // in track_ids / cts_pre_list / pts_pre_list (:742-765, :914)
    int id;        // the track-id code
    int chosen;    // id_symmetry_pre_list[idx_obj] (:926), -1 = None
    int cts_none;  // cts_pre_list's entry is None (:744)
    double cts[2];                  // cts_pre_list's entry: float32 values by box, float64 under center_3D
    float pts[2 * CP_PT_JOINTS];    // pts_pre_list's entry (NaN: the reference's None, :836, :849)
    unsigned pmask;                 // pts_mask_pre_list's entry, bit j
    unsigned pad;
};

// the tracking additions of the current-frame objects kernel (pose_targets.hip); on == 0: cp_pose_targets itself
struct PtTrackCur {
    int on, Kp, pre_hm_hp, tracking, tracking_hp;
    const double* timg;    // [B][CP_PTK_IMG_STRIDE]
    const double* cur;     // [B][K][CP_PTK_CUR_STRIDE]
    const PtkPreOut* pre;  // [B][Kp]
    float* out_tracking;
    unsigned char* out_tracking_mask;
    float* out_tracking_hp;
    unsigned char* out_tracking_hp_mask;
};

// one previous object's result; draws[c][0] is channel c's own Gaussian, draws[c][1] its false positive (c = 0: the
// centre on pre_hm, c = 1 + j: joint j on pre_hm_hp)
struct PtkPre {
    PtkPreOut o;
    int radius;
    int draw_on[1 + CP_PT_JOINTS][2];
    int draw_xy[1 + CP_PT_JOINTS][2][2];
    double draw_k[1 + CP_PT_JOINTS][2];
};

// a draw's coordinate for the int draw list; a centre a billion pixels out covers nothing either way
PT_HD int ptk_coord(long long v) { return (int)(v > 1000000000 ? 1000000000 : (v < -1000000000 ? -1000000000 : v)); }

// np.maximum(1 - 2 ** (np.sqrt(nx ** 2 + ny ** 2) - 4.5), 0) (:819, :922)
PT_HD double ptk_heat(double nx, double ny) {
    const double v = 1 - ptk_pow(2.0, sqrt(ptk_pow(nx, 2.0) + ptk_pow(ny, 2.0)) - 4.5);
    return v > 0 ? v : 0.0;  // np.maximum propagates a NaN; the truncated normals are finite
}

// what ptk_pre_object and ptk_pre_object_det (pose_targets_track_det_common.h) share of one previous object: the points,
// the box and the noisy centre (:575-720)
struct PtkGeo {
    long long pi[8][2];  // pts_pre[:, :2] before the joints' affine
    int vis[8];
    int idsym, radius;
    double w, h;
    double nx, ny;         // the centre's noise (:715)
    double ct0[2], ct[2];  // the centre and the noisy centre: float32 values by box, float64 under center_3D
};

PT_HD void ptk_pre_clear(const double* pre, PtkPre* res) {
    PtkPreOut& o = res->o;
    o.kept = 0, o.id = (int)pre[CP_PTK_PRE_ID], o.chosen = -1, o.cts_none = 1, o.cts[0] = o.cts[1] = 0.0, o.pmask = 0, o.pad = 0;
    for (int i = 0; i < 2 * CP_PT_JOINTS; ++i) o.pts[i] = 0.f;
    res->radius = 0;
    for (int c = 0; c < 1 + CP_PT_JOINTS; ++c) res->draw_on[c][0] = res->draw_on[c][1] = 0;
}

// `img` has pose_targets_common.h's image layout with the PREVIOUS frame's affine (trans_input_pre) and projection
// matrix in it; `pre` is one previous-object record; S the category's variant count (theta = 2 pi / S).  Returns false
// for an object that the cup / mug filter or the box and visibility tests of :641 drop.
PT_HD bool ptk_pre_geometry(const double* img, const double* pre, int S, const PtkOpts& op, PtkGeo* g) {
    if (pre[CP_PTK_PRE_SKIP] != 0.0) return false;  // the cup / mug filter (:567-571)
    const double* tr = img + CP_PT_IMG_TRANS;
    const double* dw = pre + CP_PTK_PRE_DRAWS;
    const double width = img[CP_PT_IMG_WIDTH], height = img[CP_PT_IMG_HEIGHT];
    const bool flipped = img[CP_PT_IMG_FLIPPED] != 0.0;
    const int idsym = (int)pre[CP_PTK_PRE_IDSYM];
    g->idsym = idsym;
    long long (*pi)[2] = g->pi;
    int* vis = g->vis;
    // the 9 points, visibility, flip: as the current frame's (:575-626)
    double p[9][2];
    if ((int)pre[CP_PT_OBJ_NSYM] != 1) {
        long long q[9][2];
        pt_project(img, pre, idsym, S, q);
        for (int i = 0; i < 9; ++i) p[i][0] = (double)q[i][0], p[i][1] = (double)q[i][1];
    } else {
        for (int i = 0; i < 9; ++i) p[i][0] = pre[CP_PT_OBJ_CUBOID + 2 * i], p[i][1] = pre[CP_PT_OBJ_CUBOID + 2 * i + 1];
    }
    int vsum = 0;
    for (int i = 0; i < 8; ++i) {
        const double x = p[i + 1][0], y = p[i + 1][1];
        vis[i] = (x >= width || x < 0 || y < 0 || y >= height) ? 1 : 2;
        vsum += vis[i];
        pi[i][0] = pt_trunc(x);
        pi[i][1] = pt_trunc(y);
    }
    if (flipped) {
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
    // bounding_box_rotation through trans_input_pre, clipped to the input (:628-633)
    double bb[4];
    for (int i = 0; i < 8; ++i) {
        double x, y;
        pt_affine(tr, (double)pi[i][0], (double)pi[i][1], &x, &y);
        if (i == 0 || x < bb[0]) bb[0] = x;
        if (i == 0 || y < bb[1]) bb[1] = y;
        if (i == 0 || x > bb[2]) bb[2] = x;
        if (i == 0 || y > bb[3]) bb[3] = y;
    }
    const double hx = (double)(op.input_w - 1), hy = (double)(op.input_h - 1);
    bb[0] = bb[0] < 0.0 ? 0.0 : (bb[0] > hx ? hx : bb[0]);
    bb[2] = bb[2] < 0.0 ? 0.0 : (bb[2] > hx ? hx : bb[2]);
    bb[1] = bb[1] < 0.0 ? 0.0 : (bb[1] > hy ? hy : bb[1]);
    bb[3] = bb[3] < 0.0 ? 0.0 : (bb[3] > hy ? hy : bb[3]);
    const double h = bb[3] - bb[1], w = bb[2] - bb[0];
    const double cx0 = p[0][0], cy0 = p[0][1];
    const bool visible = !((cx0 >= width || cx0 < 0 || cy0 < 0 || cy0 >= height) && vsum <= 12);  // :636-639
    if (!(((h > 0 && w > 0) || img[CP_PT_IMG_ROT] != 0.0) && visible)) return false;
    const double rr = pt_gaussian_radius(ceil(h), ceil(w));
    const int radius = rr > 0 ? (int)rr : 0;
    g->radius = radius, g->w = w, g->h = h;
    // the centre, its noise and its truncation (:698-720): a float32 array by box, float64 under center_3D
    const double nx = dw[CP_PTK_DRAW_CT_NOISE], ny = dw[CP_PTK_DRAW_CT_NOISE + 1];
    double* ct0 = g->ct0;
    double* ct = g->ct;
    g->nx = nx, g->ny = ny;
    if (!op.center_3D) {
        ct0[0] = (double)(float)((bb[0] + bb[2]) / 2), ct0[1] = (double)(float)((bb[1] + bb[3]) / 2);
        ct[0] = (double)(float)(ct0[0] + nx * op.hm_disturb * w);
        ct[1] = (double)(float)(ct0[1] + ny * op.hm_disturb * h);
    } else {
        pt_affine(tr, flipped ? width - cx0 - 1 : cx0, cy0, &ct0[0], &ct0[1]);
        ct[0] = ct0[0] + nx * op.hm_disturb * w;
        ct[1] = ct0[1] + ny * op.hm_disturb * h;
    }
    return true;
}

PT_HD void ptk_pre_object(const double* img, const double* pre, int S, const PtkOpts& op, PtkPre* res) {
    PtkPreOut& o = res->o;
    ptk_pre_clear(pre, res);
    PtkGeo g;
    if (!ptk_pre_geometry(img, pre, S, op, &g)) return;
    const double* tr = img + CP_PT_IMG_TRANS;
    const double* dw = pre + CP_PTK_PRE_DRAWS;
    const long long (*pi)[2] = g.pi;
    const int* vis = g.vis;
    const int idsym = g.idsym, radius = g.radius;
    const double w = g.w, h = g.h, nx = g.nx, ny = g.ny;
    const double* ct0 = g.ct0;
    const double* ct = g.ct;
    res->radius = radius;
    const long long cix = pt_trunc(ct[0]), ciy = pt_trunc(ct[1]);
    // the noisy centre left the input: the object is in none of the lists (:725-727)
    if (cix >= op.input_w || ciy >= op.input_h || cix < 0 || ciy < 0) return;
    double conf = 0.0;  // :730-737
    if (dw[CP_PTK_DRAW_CT_LOST] > op.lost_disturb) conf = op.hm_heat_random ? dw[CP_PTK_DRAW_CT_HEAT] : 1.0;
    const double dr = (double)op.down_ratio;
    const double* lab = (conf == 0.0 || op.tracking_label_mode != 0) ? ct : ct0;  // :739-750
    o.cts_none = conf == 0.0 && op.tracking_label_mode != 0;
    for (int i = 0; i < 2; ++i) {
        const double v = lab[i] / dr;  // a float32 division by box (exact through float64), float64 under center_3D
        o.cts[i] = o.cts_none ? 0.0 : (op.center_3D ? v : (double)(float)v);
    }
    o.kept = 1;
    // hm_pre[...] = 0.9999 at :773 is dead code: the visibility flags are 1 or 2, so pts_pre[:, 2].sum() is never 0.
    for (int j = 0; j < CP_PT_JOINTS; ++j) {  // :787-888
        const double* dj = dw + CP_PTK_DRAW_JOINTS + CP_PTK_DRAW_JOINT_STRIDE * j;
        double x, y;
        pt_affine(tr, (double)pi[j][0], (double)pi[j][1], &x, &y);
        const long long jx = pt_trunc(x), jy = pt_trunc(y);  // assigned back into int64
        if (!(vis[j] > 1 && jx >= 0 && jx < op.input_w && jy >= 0 && jy < op.input_h)) continue;
        const double jnx = dj[CP_PTK_DRAW_J_NOISE], jny = dj[CP_PTK_DRAW_J_NOISE + 1];
        const long long qx = pt_trunc((double)jx + jnx * op.hm_hp_disturb * w);  // the noise added into int64 (:810-811)
        const long long qy = pt_trunc((double)jy + jny * op.hm_hp_disturb * h);
        double conf_hp = 0.0;  // :814-823
        if (dj[CP_PTK_DRAW_J_LOST] > op.hp_lost_disturb) conf_hp = op.hm_hp_heat_random ? ptk_heat(jnx, jny) : 1.0;
        // the label (:830-850): float32 of the int64 point, / down_ratio in float32 (:914)
        int mode;  // 0: the ground truth pt0, 1: the noisy point, 2: None
        if (conf_hp == 0.0) mode = op.tracking_label_mode == 0 ? 1 : 2;
        else mode = op.tracking_label_mode == 0 ? 0 : (conf != 0.0 ? 1 : 2);
        if (mode == 2) {
            o.pts[2 * j] = o.pts[2 * j + 1] = NAN;
        } else {
            o.pts[2 * j] = (float)((double)(float)(mode == 0 ? jx : qx) / dr);
            o.pts[2 * j + 1] = (float)((double)(float)(mode == 0 ? jy : qy) / dr);
            o.pmask |= 1u << j;
        }
        if (op.pre_hm_hp && conf != 0.0) {  // a lost centre draws no joint (:874)
            res->draw_on[1 + j][0] = 1;
            res->draw_xy[1 + j][0][0] = ptk_coord(qx), res->draw_xy[1 + j][0][1] = ptk_coord(qy);
            res->draw_k[1 + j][0] = conf_hp;
            if (dj[CP_PTK_DRAW_J_FP] < op.hp_fp_disturb) {  // pt2 is int64 as pt0 is (:879-883)
                res->draw_on[1 + j][1] = 1;
                res->draw_xy[1 + j][1][0] = ptk_coord(pt_trunc((double)jx + dj[CP_PTK_DRAW_J_FP_NOISE] * 0.05 * w));
                res->draw_xy[1 + j][1][1] = ptk_coord(pt_trunc((double)jy + dj[CP_PTK_DRAW_J_FP_NOISE + 1] * 0.05 * h));
                res->draw_k[1 + j][1] = dj[CP_PTK_DRAW_J_FP_PEAK];
            }
        }
    }
    if (op.pre_hm) {  // :918-937
        if (conf != 0.0 && op.hm_heat_random) conf = ptk_heat(nx, ny);  // the late re-evaluation (:922)
        res->draw_on[0][0] = 1;
        res->draw_xy[0][0][0] = (int)cix, res->draw_xy[0][0][1] = (int)ciy;
        res->draw_k[0][0] = conf;
        if (conf != 0.0) o.chosen = idsym;
        if (dw[CP_PTK_DRAW_CT_FP] < op.fp_disturb) {  // ct2 has ct0's dtype (:930-934)
            double c2x = ct0[0] + dw[CP_PTK_DRAW_CT_FP_NOISE] * 0.05 * w, c2y = ct0[1] + dw[CP_PTK_DRAW_CT_FP_NOISE + 1] * 0.05 * h;
            if (!op.center_3D) c2x = (double)(float)c2x, c2y = (double)(float)c2y;
            res->draw_on[0][1] = 1;
            res->draw_xy[0][1][0] = ptk_coord(pt_trunc(c2x)), res->draw_xy[0][1][1] = ptk_coord(pt_trunc(c2y));
            res->draw_k[0][1] = dw[CP_PTK_DRAW_CT_FP_PEAK];
        }
    }
}

#ifdef __HIPCC__
// What the previous-objects kernels pass to ptk_pre_object as `img`: image b's current record with the previous frame's
// affine and projection matrix in it, into im[CP_PT_IMG_STRIDE].  Returns the image's count of previous objects.
__device__ __forceinline__ int ptk_pre_image(const double* __restrict__ img, const double* __restrict__ timg, int b, double* im) {
    const double* ti = timg + (size_t)b * CP_PTK_IMG_STRIDE;
    for (int i = 0; i < CP_PT_IMG_STRIDE; ++i) im[i] = img[(size_t)b * CP_PT_IMG_STRIDE + i];
    for (int i = 0; i < 6; ++i) im[CP_PT_IMG_TRANS + i] = ti[CP_PTK_IMG_TRANS + i];
    for (int i = 0; i < 16; ++i) im[CP_PT_IMG_PROJ + i] = ti[CP_PTK_IMG_PROJ + i];
    return (int)ti[CP_PTK_IMG_NUM_PRE];
}

// One wavefront, lane k = previous object k of image b: compacts the Gaussians to draw, per channel, into the image's
// lists as (x, y, r, 0) and a peak, with ballots in object order, an object's own draws before the false positives; a
// draw with k == 0 adds nothing to a map of non-negative values and is dropped.  Every lane of the wavefront calls it.
__device__ __forceinline__ void ptk_emit_draws(const PtkPre& r, int b, int k, int Kp, int* __restrict__ counts,
                                               int4* __restrict__ draws, double* __restrict__ peaks) {
    constexpr int nch = 1 + CP_PT_JOINTS;
    const unsigned long long below = (1ull << k) - 1;
    for (int c = 0; c < nch; ++c) {
        int base = 0;
        for (int f = 0; f < 2; ++f) {
            const bool v = r.draw_on[c][f] && r.draw_k[c][f] != 0.0;
            const unsigned long long m = __ballot(v);
            if (v) {
                const size_t at = ((size_t)b * nch + c) * 2 * Kp + base + __popcll(m & below);
                draws[at] = make_int4(r.draw_xy[c][f][0], r.draw_xy[c][f][1], r.radius, 0);
                peaks[at] = r.draw_k[c][f];
            }
            base += __popcll(m);
        }
        if (k == 0) counts[b * nch + c] = base;
    }
}
#endif

}  // namespace pose_targets

#if defined(__clang__) && defined(__HIPCC__)
#pragma clang fp contract(fast)  // hipcc's default again for whatever the including file defines after this header
#endif
