// The scalar logic of pose_targets_track_det.hip: the tracking task's previous-frame targets with a trained detector in
// the loop, ObjectPoseDataset.__getitem__ with data_generation_mode == 1 (datasets/dataset_combined.py:464-550 the
// matching of the detector's boxes to the annotations, :644-693, :752-763, :792-794, :851-867, :890-911, :939-952 the
// branches of the per-object loop), written so that the host compiler can build it too
// (tests/native/pose_targets_track_det_host.cpp; tests/test_pose_targets_track_det_cpu.py pins it to the numpy
// restatement tests/pose_targets_track_det_ref.py).  What the detector's boxes are made of, pnp_shell's packaging and
// rejects (utils/pnp/cuboid_pnp_shell.py:46-88), is track_common.h's trk_shell_pnp / trk_shell_ori; the object's points,
// box and noisy centre are pose_targets_track_common.h's ptk_pre_geometry, shared with the noise-simulation mode.
#pragma once
#include "pose_targets_track_common.h"
#include "track_common.h"  // (leaves fused multiply-adds off for the rest of this header)

// the host record per image (include/centerpose_hip.h), repeated as pose_targets_track_common.h repeats its own
#define CP_PTKD_GEN_STRIDE 4
#define CP_PTKD_GEN_MODE 0
#define CP_PTKD_GEN_RADIUS_SCALE 1
#define CP_PTKD_MAX_K 128

// what the matching leaves per previous object for the objects kernel (workspace, float64)
#define PTKD_STRIDE 64
#define PTKD_SLOT 0     // the matched slot of the post / pnp records, -1: no box (match_detector_idx None, :645-661)
#define PTKD_SCORE 1    // result_ori['score'] as :949-951 read it: the score of the image's LAST box
#define PTKD_CT 2       // [2]  box[4]['ct'] (:665)
#define PTKD_PNP 4      // [16] box[0][1:], the reprojected vertices, normalised (:674)
#define PTKD_ORI 20     // [16] box[3][1:], kps_ori's vertices, normalised (:671)
#define PTKD_STD 36     // [16] box[4]['kps_heatmap_std'], float32 values (:683)
#define PTKD_HEIGHT 52  // [8]  box[4]['kps_heatmap_height'], float32 values (:693)
#define PTKD_NORM 60    // the matched box's norm to this object
#define PTKD_OWN_SCORE 61  // the matched box's own score (not read by the targets)

namespace pose_targets {

struct PtkDetOpts {
    int render_hm_mode, render_hmhp_mode, cat_rule;
};

// a slot of cp_pnp_from_post is a box when the solve succeeded (base_detector.py:652-654 with the solver's rejects in the
// status) and pnp_shell's rejects pass; pnp9 [18]: box[0], the 9 normalised reprojected points
CP_HD int ptkd_box(int cat_rule, double width, double height, const double* pnp_row, double* pnp9) {
    if ((int)pnp_row[0] != 1) return 0;
    return trk_shell_pnp(cat_rule, width, height, pnp_row, pnp9);
}

// instances_2d's entry of one previous object (:506-532), rows 1..8 into inst [16].  float32 throughout: the cuboid is
// cast first and width / height are Python ints.  flip_idx - 1 is applied to the nine-row array, so the centre trades
// places with row 4 before the visibility test and the norms read it.
CP_HD void ptkd_instance(const double* img, const double* pre, double* inst) {
    float c[9][2];
    for (int i = 0; i < 9; ++i) c[i][0] = (float)pre[CP_PT_OBJ_CUBOID + 2 * i], c[i][1] = (float)pre[CP_PT_OBJ_CUBOID + 2 * i + 1];
    const float width = (float)img[CP_PT_IMG_WIDTH], height = (float)img[CP_PT_IMG_HEIGHT];
    if (img[CP_PT_IMG_FLIPPED] != 0.0) {
        for (int i = 0; i < 9; ++i) c[i][0] = width - c[i][0] - 1.0f;
        const int sw[4][2] = {{0, 4}, {2, 6}, {1, 5}, {3, 7}};
        for (int e = 0; e < 4; ++e)
            for (int d = 0; d < 2; ++d) {
                const float t = c[sw[e][0]][d];
                c[sw[e][0]][d] = c[sw[e][1]][d];
                c[sw[e][1]][d] = t;
            }
    }
    for (int i = 0; i < 9; ++i) c[i][0] = c[i][0] / width, c[i][1] = c[i][1] / height;
    const bool visible = c[0][0] > 0 && c[0][0] < 1 && c[0][1] > 0 && c[0][1] < 1;
    for (int i = 0; i < 8; ++i) {
        inst[2 * i] = visible ? (double)c[i + 1][0] : -10000.0;
        inst[2 * i + 1] = visible ? (double)c[i + 1][1] : -10000.0;
    }
}

// np.linalg.norm(instances_2d[o, 1:, :] - box_point_2d[1:, :]) (:542): float64, the 16 squares summed in row order
CP_HD double ptkd_norm(const double* inst, const double* pnp9) {
    double s = 0.0;
    for (int i = 0; i < 16; ++i) {
        const double d = inst[i] - pnp9[2 + i];
        s += d * d;
    }
    return sqrt(s);
}

// np.argmin's step: does `n` replace the running minimum `best`?  The first NaN wins and stays.
CP_HD bool ptkd_takes(double n, double best) { return best == best && (n != n || n < best); }

// the box of previous object o (:646-661) among K slots: amin[k] is the object that slot k's norms are smallest for (-1:
// the slot is no box), nmin[k] that norm.  The only such box is taken whatever its norm; among several the nearest, the
// lowest slot on ties, and none when even that one is farther than 1000.
CP_HD int ptkd_select(const int* amin, const double* nmin, int K, int o, double* norm) {
    int cnt = 0, best = -1;
    double bn = 0.0;
    for (int k = 0; k < K; ++k) {
        if (amin[k] != o) continue;
        if (cnt == 0 || ptkd_takes(nmin[k], bn)) best = k, bn = nmin[k];
        ++cnt;
    }
    *norm = bn;
    if (cnt > 1 && bn > 1000) return -1;
    return best;
}

// the match record of one previous object from its box's rows (slot < 0: no box)
CP_HD void ptkd_fill(int slot, double norm, double last_score, int cat_rule, double width, double height, const double* post_row,
                     const double* pnp_row, double* m) {
    for (int i = 0; i < PTKD_STRIDE; ++i) m[i] = 0.0;
    m[PTKD_SLOT] = (double)slot;
    m[PTKD_SCORE] = last_score;
    if (slot < 0) return;
    double p9[18];
    ptkd_box(cat_rule, width, height, pnp_row, p9);
    for (int i = 0; i < 16; ++i) m[PTKD_PNP + i] = p9[2 + i];
    trk_shell_ori(width, height, post_row + PO_KPS, p9);
    for (int i = 0; i < 16; ++i) m[PTKD_ORI + i] = p9[2 + i];
    m[PTKD_CT] = post_row[PO_CT], m[PTKD_CT + 1] = post_row[PO_CT + 1];
    for (int i = 0; i < 16; ++i) m[PTKD_STD + i] = (double)(float)post_row[PO_HM_STD + i];
    for (int i = 0; i < 8; ++i) m[PTKD_HEIGHT + i] = (double)(float)post_row[PO_HM_HEIGHT + i];
    m[PTKD_NORM] = norm;
    m[PTKD_OWN_SCORE] = post_row[PO_SCORE];
}

// The whole matching of one image, one slot and one object after the other: what det_boxes_match_kernel computes with a
// lane per slot and then a lane per object.  post / pnp: the image's K_det rows; match: [npre][PTKD_STRIDE].
CP_HD void ptkd_match_image(const double* img, const double* pre, int npre, int cat_rule, const double* post,
                            const double* pnp, int count, int K_det, double* match) {
    int amin[CP_PTKD_MAX_K];
    double nmin[CP_PTKD_MAX_K];
    const double width = img[CP_PT_IMG_WIDTH], height = img[CP_PT_IMG_HEIGHT];
    const int n = count < 0 ? 0 : (count > K_det ? K_det : count);
    int last = -1;
    for (int k = 0; k < K_det; ++k) {
        double p9[18], inst[16];
        amin[k] = -1, nmin[k] = 0.0;
        if (k >= n || !ptkd_box(cat_rule, width, height, pnp + (size_t)k * 40, p9)) continue;
        last = k;
        for (int o = 0; o < npre; ++o) {
            ptkd_instance(img, pre + (size_t)o * CP_PTK_PRE_STRIDE, inst);
            const double v = ptkd_norm(inst, p9);
            if (o == 0 || ptkd_takes(v, nmin[k])) amin[k] = o, nmin[k] = v;
        }
    }
    const double last_score = last >= 0 ? post[(size_t)last * 120 + PO_SCORE] : 0.0;
    for (int o = 0; o < npre; ++o) {
        double norm;
        const int s = ptkd_select(amin, nmin, K_det, o, &norm);
        ptkd_fill(s, norm, last_score, cat_rule, width, height, post + (size_t)(s < 0 ? 0 : s) * 120,
                  pnp + (size_t)(s < 0 ? 0 : s) * 40, match + (size_t)o * PTKD_STRIDE);
    }
}

// astype(np.int32) of a float64 (:682-690); outside int32 the conversion gives INT_MIN, as cvttsd2si does
CP_HD int ptkd_int32(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : (-2147483647 - 1); }

// One previous object of an image in data_generation_mode 1.  `img`, `pre`, S, op: as ptk_pre_object's; `m`: the object's
// match record; radius_scale: aug_s or aug_s_pre (:681-690).
CP_HD void ptk_pre_object_det(const double* img, const double* pre, const double* m, double radius_scale, int S,
                              const PtkOpts& op, const PtkDetOpts& dop, PtkPre* res) {
    PtkPreOut& o = res->o;
    ptk_pre_clear(pre, res);
    PtkGeo g;
    if (!ptk_pre_geometry(img, pre, S, op, &g)) return;
    res->radius = g.radius;
    const double* tr = img + CP_PT_IMG_TRANS;
    const double* dw = pre + CP_PTK_PRE_DRAWS;
    const double width = img[CP_PT_IMG_WIDTH], height = img[CP_PT_IMG_HEIGHT];
    const double dr = (double)op.down_ratio;
    const bool matched = m[PTKD_SLOT] >= 0.0;
    double ctd[2] = {0.0, 0.0};  // ct_detector (:665-666)
    if (matched) pt_affine(tr, m[PTKD_CT], m[PTKD_CT + 1], &ctd[0], &ctd[1]);
    // cts_pre_list (:752-763): the test of :725-727 belongs to mode 0, the object stays wherever the noisy centre went
    o.cts_none = !matched && op.tracking_label_mode != 0;
    for (int i = 0; i < 2; ++i) {
        double v;
        if (matched && op.tracking_label_mode != 0) v = ctd[i] / dr;  // a float64 array
        else {
            v = (matched ? g.ct0[i] : g.ct[i]) / dr;  // float32 by box, float64 under center_3D, as in mode 0
            if (!op.center_3D) v = (double)(float)v;
        }
        o.cts[i] = o.cts_none ? 0.0 : v;
    }
    o.kept = 1;
    // pts_detector (:669-678): kps_ori's vertices or the reprojected ones, * (width, height) in float64
    const double* src = m + (dop.render_hmhp_mode < 2 ? PTKD_ORI : PTKD_PNP);
    for (int j = 0; j < CP_PT_JOINTS; ++j) {
        const double* dj = dw + CP_PTK_DRAW_JOINTS + CP_PTK_DRAW_JOINT_STRIDE * j;
        double x, y, px = 0.0, py = 0.0;
        pt_affine(tr, (double)g.pi[j][0], (double)g.pi[j][1], &x, &y);
        if (matched) pt_affine(tr, src[2 * j] * width, src[2 * j + 1] * height, &px, &py);  // :792-794
        const long long jx = pt_trunc(x), jy = pt_trunc(y);
        if (!(g.vis[j] > 1 && jx >= 0 && jx < op.input_w && jy >= 0 && jy < op.input_h)) continue;
        // the noise is still added into the int64 point (:810-811); the lost uniform of :814 decides nothing here
        const long long qx = pt_trunc((double)jx + dj[CP_PTK_DRAW_J_NOISE] * op.hm_hp_disturb * g.w);
        const long long qy = pt_trunc((double)jy + dj[CP_PTK_DRAW_J_NOISE + 1] * op.hm_hp_disturb * g.h);
        if (!matched && op.tracking_label_mode != 0) {  // :853-860
            o.pts[2 * j] = o.pts[2 * j + 1] = NAN;
        } else {
            double lx, ly;  // the float32 pts_single_pre entry, / down_ratio in float32 (:914)
            if (!matched) lx = (double)(float)qx, ly = (double)(float)qy;
            else if (op.tracking_label_mode == 0) lx = (double)(float)jx, ly = (double)(float)jy;
            else lx = (double)(float)px, ly = (double)(float)py;
            o.pts[2 * j] = (float)(lx / dr);
            o.pts[2 * j + 1] = (float)(ly / dr);
            o.pmask |= 1u << j;
        }
        if (op.pre_hm_hp && matched && px >= 0 && px < op.input_w && py >= 0 && py < op.input_h) {  // :890-911
            double k = 1.0;
            bool on = true;
            if (!(dop.render_hmhp_mode & 1)) {
                on = ptkd_int32(m[PTKD_STD + 2 * j] * radius_scale) > 0;  // radius_detector[j, 0]
                k = m[PTKD_HEIGHT + j];
            }
            if (on) {
                res->draw_on[1 + j][0] = 1;
                res->draw_xy[1 + j][0][0] = (int)px, res->draw_xy[1 + j][0][1] = (int)py;
                res->draw_k[1 + j][0] = k;
            }
        }
    }
    if (op.pre_hm && matched) {  // :939-952, no bounds test on ct_detector
        const double k = dop.render_hm_mode == 0 ? 1.0 : m[PTKD_SCORE];
        res->draw_on[0][0] = 1;
        res->draw_xy[0][0][0] = ptk_coord(pt_trunc(ctd[0])), res->draw_xy[0][0][1] = ptk_coord(pt_trunc(ctd[1]));
        res->draw_k[0][0] = k;
        if (dop.render_hm_mode == 0 || k != 0.0) o.chosen = g.idsym;
    }
}

}  // namespace pose_targets

#if defined(__clang__) && defined(__HIPCC__)
#pragma clang fp contract(fast)  // hipcc's default again for whatever the including file defines after this header
#endif
