// The float64 numerics of the Objectron box metrics (box3d.hip), written so that the host compiler can build them too
// (tests/native/box3d_host.cpp, tests/test_box_metrics_cpu.py pins them to the reference evaluator's own output,
// tests/golden/box_eval_ref.npz).  Every routine restates one routine of the reference's evaluator:
//   objectron/dataset/box.py      Box.fit :130-163, volume :214-231, inside :165-183, transformation /
//                                 apply_transformation :91-110 + :233-241
//   objectron/dataset/iou.py      IoU.iou :22-37, _compute_intersection_points :75-94, Sutherland-Hodgman :96-211
//   eval_image_official.py        evaluate_2d :673-719, _get_rotated_box :721-737, evaluate_3d :739-793,
//                                 compute_ray / compute_average_distance / compute_viewpoint / evaluate_viewpoint :864-994
// The one deliberate departure is the intersection volume: the reference takes scipy's ConvexHull of the clipped points
// (qhull); here it is the divergence theorem over the clipped faces of both boxes (box_iou below).
#pragma once
#include <cmath>

// Same record layout as include/centerpose_hip.h, repeated so that the host build needs no other header (an identical
// redefinition is legal, a drifting one is a compile error).
#define CP_BOX_EVAL_STRIDE 9
#define CP_BOX_FLAG_SINGULAR_RAY 1
#define CP_BOX_FLAG_SINGULAR_MO2C 2
#define CP_BOX_FLAG_CLIP_OVERFLOW 4

// No fused multiply-adds in either build: the arithmetic restates numpy expressions whose every operation rounds, and the
// host build of this source must pin what the device computes.  Restored at the end of the header.
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#ifdef __HIPCC__
#define BOX_HD __host__ __device__ inline
#else
#define BOX_HD static inline
#endif

namespace box3d {

constexpr double PLANE_EPS = 0.000001;  // iou.py:8 _PLANE_THICKNESS_EPSILON
constexpr double MAX_DISTANCE = 1.0;    // eval_image_official.py:63 _MAX_DISTANCE
constexpr double TWO_PI = 6.283185307179586;  // np.pi * 2
// A face (4 vertices) clipped by the 6 planes of a convex box keeps at most 4 + 6 vertices: each Sutherland-Hodgman
// pass over a convex polygon adds at most one (two strict crossings, every kept vertex emitted once).  The reference
// emits one vertex twice: an on-plane LAST vertex is emitted as `prev` at i = 0 and again as `cur` at i = n - 1, and its
// array_equal test only looks at the previous output.  That copy is output[0] repeated at the end of the cycle -- a
// zero-length closing edge, the same polygon and the same point set for the hull -- and clip_poly leaves it out, which
// keeps the bound at one vertex per pass.  Writes past the capacity would be dropped and flagged (CLIP_OVERFLOW).
constexpr int MAXV = 10;

// Box.FACES (box.py:22-29) packed 4 bits per vertex, face f in bits [16 f, 16 f + 16): register-resident, so a runtime
// face index never sends a table to scratch memory.
constexpr unsigned long long FACES_LO = 0x7865ULL | (0x2431ULL << 16) | (0x4873ULL << 32) | (0x5621ULL << 48);
constexpr unsigned long long FACES_HI = 0x6842ULL | (0x3751ULL << 16);
BOX_HD int face_vertex(int f, int k) {
    const unsigned long long w = f < 4 ? (FACES_LO >> (16 * f)) : (FACES_HI >> (16 * (f - 4)));
    return (int)((w >> (4 * k)) & 15ULL);
}

// Box vertex i of scaled_axis_aligned_vertices (box.py:119-127): vertex i >= 1 has, in the bits of i - 1, x at bit 2,
// y at bit 1, z at bit 0 (set = +half extent).
BOX_HD double aabb_coord(const double s[3], int i, int c) {
    if (i == 0) return 0.0;
    const double h = s[c] / 2.;
    return ((i - 1) >> (2 - c)) & 1 ? h : -h;
}

struct Fit {
    double R[9];  // "rotation": the lstsq 3 x 3, NOT re-orthogonalised (noisy vertices give a general matrix, as upstream)
    double t[3];
    double s[3];
};

BOX_HD double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// Box.fit (box.py:130-163).  Scale: the mean of the 4 edge lengths per axis (EDGES).  Orientation and translation:
// lstsq of [scaled unit box | 1] (9 x 4) against the 9 vertices.  The 9 model rows are centred (row 0 is the origin) and
// sign-balanced (every pair of axes has as many equal as opposite signs over the 8 corners), so the normal matrix is
// diag(2 s_x^2, 2 s_y^2, 2 s_z^2, 9) and the least-squares solution is exact in closed form:
//   row k < 3 of the solution = sum_i x_ik v_i / (2 s_k^2),  row 3 = sum_i v_i / 9.
// An axis of zero extent has a zero column; lstsq's minimum-norm solution leaves its row 0, so does this.
BOX_HD void box_fit(const double* v, Fit& f) {
    const int eb[12] = {1, 2, 3, 4, 1, 5, 2, 6, 1, 3, 5, 7};
    const int ee[12] = {5, 6, 7, 8, 3, 7, 4, 8, 2, 4, 6, 8};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double sc = 0.;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int b = eb[a * 4 + e], d = ee[a * 4 + e];
            sc += norm3(v[b * 3] - v[d * 3], v[b * 3 + 1] - v[d * 3 + 1], v[b * 3 + 2] - v[d * 3 + 2]);
        }
        f.s[a] = sc / 4.;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double den = 2. * (f.s[k] * f.s[k]);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double acc = 0.;
#pragma unroll
            for (int i = 1; i < 9; ++i) acc += aabb_coord(f.s, i, k) * v[i * 3 + j];
            f.R[j * 3 + k] = den > 0. ? acc / den : 0.;  // orientation = solution[:3, :3].T
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double acc = 0.;
#pragma unroll
        for (int i = 0; i < 9; ++i) acc += v[i * 3 + j];
        f.t[j] = acc / 9.;
    }
}

// vertex i of Box.from_transformation(R, t, s) (box.py:63-75): R @ aabb(s)[i] + t
BOX_HD void box_vertex(const double R[9], const double t[3], const double s[3], int i, double o[3]) {
    const double a0 = aabb_coord(s, i, 0), a1 = aabb_coord(s, i, 1), a2 = aabb_coord(s, i, 2);
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = R[r * 3] * a0 + R[r * 3 + 1] * a1 + R[r * 3 + 2] * a2 + t[r];
}

// Box.volume (box.py:214-231): |det(v2 - v1, v3 - v1, v5 - v1)| of the vertices as given (not of the fitted box)
BOX_HD double box_volume(const double* v) {
    double m[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        m[c] = v[2 * 3 + c] - v[3 + c];
        m[3 + c] = v[3 * 3 + c] - v[3 + c];
        m[6 + c] = v[5 * 3 + c] - v[3 + c];
    }
    const double d = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
                     m[2] * (m[3] * m[7] - m[4] * m[6]);
    return fabs(d);
}

// inv(transformation) (box.py:233-241, np.linalg.inv of [R t; 0 1]).  The bottom row is (0, 0, 0, 1), so the general
// inverse is [R^-1, -R^-1 t] with R^-1 the general 3 x 3 inverse (R is not orthogonal in general: no transpose).  A
// singular R makes numpy raise, which the reference's evaluate_iou turns into IoU 0: returns false.
BOX_HD bool box_inverse(const Fit& f, double Ri[9], double ti[3]) {
    const double* R = f.R;
    const double c00 = R[4] * R[8] - R[5] * R[7], c01 = R[5] * R[6] - R[3] * R[8], c02 = R[3] * R[7] - R[4] * R[6];
    const double det = R[0] * c00 + R[1] * c01 + R[2] * c02;
    if (!(det != 0.)) return false;
    const double id = 1. / det;
    Ri[0] = c00 * id;
    Ri[1] = (R[2] * R[7] - R[1] * R[8]) * id;
    Ri[2] = (R[1] * R[5] - R[2] * R[4]) * id;
    Ri[3] = c01 * id;
    Ri[4] = (R[0] * R[8] - R[2] * R[6]) * id;
    Ri[5] = (R[2] * R[3] - R[0] * R[5]) * id;
    Ri[6] = c02 * id;
    Ri[7] = (R[1] * R[6] - R[0] * R[7]) * id;
    Ri[8] = (R[0] * R[4] - R[1] * R[3]) * id;
#pragma unroll
    for (int r = 0; r < 3; ++r) ti[r] = -(Ri[r * 3] * f.t[0] + Ri[r * 3 + 1] * f.t[1] + Ri[r * 3 + 2] * f.t[2]);
    return true;
}

// Box.apply_transformation (box.py:91-110) of the box `f` by [Mi, mt; 0 1]: rotation Mi @ R, translation mt + Mi @ t,
// scale unchanged
BOX_HD void box_apply(const double Mi[9], const double mt[3], const Fit& f, double R2[9], double t2[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) R2[r * 3 + c] = Mi[r * 3] * f.R[c] + Mi[r * 3 + 1] * f.R[3 + c] + Mi[r * 3 + 2] * f.R[6 + c];
        t2[r] = mt[r] + (Mi[r * 3] * f.t[0] + Mi[r * 3 + 1] * f.t[1] + Mi[r * 3 + 2] * f.t[2]);
    }
}

// Box.inside (box.py:165-183): the point in the box's own frame, |p_k| <= s_k / 2 on every axis
BOX_HD bool box_inside(const Fit& f, const double p[3]) {
    double Ri[9], ti[3];
    if (!box_inverse(f, Ri, ti)) return false;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double w = Ri[r * 3] * p[0] + Ri[r * 3 + 1] * p[1] + Ri[r * 3 + 2] * p[2] + ti[r];
        if (fabs(w) > f.s[r] / 2.) return false;
    }
    return true;
}

// ---- Sutherland-Hodgman (iou.py:96-211) on per-lane polygon buffers: vertex k, coordinate c at buf[(k * 3 + c) * st] ----
BOX_HD int classify(double coord, double plane, double normal) {
    const double sd = normal * (coord - plane);
    return sd > PLANE_EPS ? 1 : (sd < -PLANE_EPS ? -1 : 0);
}

BOX_HD void put(double* out, int st, int& m, double x, double y, double z, int& flags) {
    if (m >= MAXV) {
        flags |= CP_BOX_FLAG_CLIP_OVERFLOW;
        return;
    }
    out[(m * 3) * st] = x;
    out[(m * 3 + 1) * st] = y;
    out[(m * 3 + 2) * st] = z;
    ++m;
}

// _clip_poly: the same case analysis and output order, the same array_equal de-duplication of an on-plane previous
// vertex, the same lerp in _intersect; a polygon lying wholly on the plane comes back unchanged.  Only difference: the
// wrap-around repeat of output[0] described at MAXV is not emitted.
BOX_HD int clip_poly(const double* in, int n, double* out, int st, double plane, double normal, int axis, int& flags) {
    if (n <= 1) return 0;
    int m = 0;
    bool in_plane = true;
    for (int i = 0; i < n; ++i) {
        const int pv = (i + n - 1) % n;
        const double px = in[(pv * 3) * st], py = in[(pv * 3 + 1) * st], pz = in[(pv * 3 + 2) * st];
        const double cx = in[(i * 3) * st], cy = in[(i * 3 + 1) * st], cz = in[(i * 3 + 2) * st];
        const double pa = axis == 0 ? px : (axis == 1 ? py : pz), ca = axis == 0 ? cx : (axis == 1 ? cy : cz);
        const int d1 = classify(pa, plane, normal), d2 = classify(ca, plane, normal);
        if (d2 != 0) {
            in_plane = false;
            if (d1 == -d2) {
                const double alpha = (ca - plane) / (ca - pa);
                put(out, st, m, alpha * px + (1.0 - alpha) * cx, alpha * py + (1.0 - alpha) * cy,
                    alpha * pz + (1.0 - alpha) * cz, flags);
            } else if (d1 == 0) {
                const bool dup = m > 0 && out[((m - 1) * 3) * st] == px && out[((m - 1) * 3 + 1) * st] == py &&
                                 out[((m - 1) * 3 + 2) * st] == pz;
                if (!dup) put(out, st, m, px, py, pz, flags);
            }
            if (d2 == 1) put(out, st, m, cx, cy, cz, flags);
        } else if (d1 != 0) {
            const bool wrap_dup = i == n - 1 && m > 0 && out[0] == cx && out[st] == cy && out[2 * st] == cz;
            if (!wrap_dup) put(out, st, m, cx, cy, cz, flags);
        }
    }
    if (in_plane) {
        for (int k = 0; k < n * 3; ++k) out[k * st] = in[k * st];
        return n;
    }
    return m;
}

// unit outward normal of face f of the box (R, t, s), from its geometry: the cross product of two edges, turned away
// from the box centre (vertex 0); the FACES vertex order plays no part
BOX_HD void face_normal(const double R[9], const double t[3], const double s[3], int f, double n[3]) {
    double a[3], b[3], c[3], o[3];
    box_vertex(R, t, s, face_vertex(f, 0), a);
    box_vertex(R, t, s, face_vertex(f, 1), b);
    box_vertex(R, t, s, face_vertex(f, 3), c);
    box_vertex(R, t, s, 0, o);
    const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
    const double w0 = c[0] - a[0], w1 = c[1] - a[1], w2 = c[2] - a[2];
    double x = u1 * w2 - u2 * w1, y = u2 * w0 - u0 * w2, z = u0 * w1 - u1 * w0;
    const double out = x * (a[0] - o[0]) + y * (a[1] - o[1]) + z * (a[2] - o[2]);
    const double l = norm3(x, y, z);
    const double k = l > 0. ? (out < 0. ? -1. / l : 1. / l) : 0.;
    n[0] = x * k;
    n[1] = y * k;
    n[2] = z * k;
}

// One half of IoU._compute_intersection_points (iou.py:75-94): every face of `tmpl` clipped in the axis-aligned frame of
// `src`, mapped back to the world by src's fitted rotation and translation, and its term |A_f| n_f . (p_f - c) of the
// divergence theorem added to `acc`.  With skip_shared, a face of tmpl that lies on a face plane of src (every clipped
// vertex within PLANE_EPS of it) with the same outward normal is left out: the other half counts that patch once.
BOX_HD bool half_volume(const Fit& src, const Fit& tmpl, const double c[3], bool skip_shared, double* bufA, double* bufB,
                        int st, double& acc, int& flags) {
    double Ri[9], ti[3];
    if (!box_inverse(src, Ri, ti)) return false;
    double Rs[9], ts[3], Rt[9], tt[3];
    box_apply(Ri, ti, src, Rs, ts);  // box_src_axis_aligned
    box_apply(Ri, ti, tmpl, Rt, tt);  // template_in_src_coord
    double lo[3], hi[3];
    box_vertex(Rs, ts, src.s, 1, lo);
    box_vertex(Rs, ts, src.s, 8, hi);
    for (int f = 0; f < 6; ++f) {
        for (int k = 0; k < 4; ++k) {
            double p[3];
            box_vertex(Rt, tt, tmpl.s, face_vertex(f, k), p);
            bufA[(k * 3) * st] = p[0];
            bufA[(k * 3 + 1) * st] = p[1];
            bufA[(k * 3 + 2) * st] = p[2];
        }
        int m = 4;
        for (int a = 0; a < 3; ++a) {
            m = clip_poly(bufA, m, bufB, st, lo[a], 1.0, a, flags);
            m = clip_poly(bufB, m, bufA, st, hi[a], -1.0, a, flags);
        }
        if (m < 3) continue;  // no area
        if (skip_shared) {
            double nl[3];
            face_normal(Rt, tt, tmpl.s, f, nl);
            bool shared = false;
            for (int a = 0; a < 3 && !shared; ++a) {
                for (int side = 0; side < 2 && !shared; ++side) {
                    const double pl = side ? hi[a] : lo[a];
                    bool on = (side ? nl[a] : -nl[a]) > 1. - PLANE_EPS;
                    for (int k = 0; k < m && on; ++k) on = fabs(bufA[(k * 3 + a) * st] - pl) <= PLANE_EPS;
                    shared = on;
                }
            }
            if (shared) continue;
        }
        double n[3];
        face_normal(tmpl.R, tmpl.t, tmpl.s, f, n);
        // the clipped vertices in the world: box_src.rotation @ p + box_src.translation
        double w0[3], wp[3];
        double ax = 0., ay = 0., az = 0.;
        for (int k = 0; k < m; ++k) {
            const double q0 = bufA[(k * 3) * st], q1 = bufA[(k * 3 + 1) * st], q2 = bufA[(k * 3 + 2) * st];
            double w[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) w[r] = src.R[r * 3] * q0 + src.R[r * 3 + 1] * q1 + src.R[r * 3 + 2] * q2 + src.t[r];
            if (k == 0) {
                w0[0] = w[0], w0[1] = w[1], w0[2] = w[2];
            } else {
                const double d0 = w[0] - w0[0], d1 = w[1] - w0[1], d2 = w[2] - w0[2];
                if (k >= 2) {  // fan triangle (p0, p_{k-1}, p_k)
                    ax += wp[1] * d2 - wp[2] * d1;
                    ay += wp[2] * d0 - wp[0] * d2;
                    az += wp[0] * d1 - wp[1] * d0;
                }
                wp[0] = d0, wp[1] = d1, wp[2] = d2;
            }
        }
        const double area = fabs(ax * n[0] + ay * n[1] + az * n[2]) / 2.;
        acc += area * (n[0] * (w0[0] - c[0]) + n[1] * (w0[1] - c[1]) + n[2] * (w0[2] - c[2]));
    }
    return true;
}

// IoU.iou (iou.py:22-37) of two 9 x 3 vertex sets.  The intersection's boundary is (faces of A inside B) + (faces of B
// inside A), exactly the clipped polygons the reference collects, so V = 1/3 sum_f |A_f| n_f . (p_f - c) with n_f the
// face's outward normal, p_f any of its clipped vertices and c fixed (A's centre).  Where qhull has no volume to give
// (no points, a flat or degenerate set: touching faces of opposite normals cancel, edge or vertex contact has no area)
// the reference returns 0, so does a volume <= 1e-12 of the two boxes' (qhull's own round-off keeps flat sets flat).
// A singular fitted rotation (numpy raises in inv, evaluate_iou returns 0) also gives 0.
BOX_HD double box_iou(const double* a, const double* b, double* bufA, double* bufB, int st, int& flags) {
    Fit fa, fb;
    box_fit(a, fa);
    box_fit(b, fb);
    double acc = 0.;
    if (!half_volume(fa, fb, fa.t, true, bufA, bufB, st, acc, flags)) return 0.;
    if (!half_volume(fb, fa, fa.t, false, bufA, bufB, st, acc, flags)) return 0.;
    const double inter = acc / 3.;
    const double v1 = box_volume(a), v2 = box_volume(b);
    if (!(inter > 1e-12 * (v1 + v2))) return 0.;
    return inter / (v1 + v2 - inter);
}

// ---- evaluate_3d's symmetry rotation (eval_image_official.py:721-737, :767) ----
// np.linspace(0, 2 pi, n)[r]: r * step with step = 2 pi / (n - 1), the last sample exactly 2 pi
BOX_HD double sweep_angle(int r, int n) {
    if (n <= 1) return 0.;
    if (r == n - 1) return TWO_PI;
    return (double)r * (TWO_PI / (double)(n - 1));
}

// Rotation.from_rotvec(angle * up / |up|).as_dcm() as scipy evaluates it -- Rodrigues' rotation written through the
// half-angle quaternion (x, y, z, w) = (sin(|r|/2) / |r| * r, cos(|r|/2)), with scipy's series below |r| = 1e-3 --
// applied as (v - v[0]) @ R + v[0] (R transposed on column vectors).
BOX_HD void rotate_box(const double* v, double theta, double* o) {
    const double u0 = v[9] - v[3], u1 = v[10] - v[4], u2 = v[11] - v[5];
    const double un = norm3(u0, u1, u2);
    const double r0 = theta * u0 / un, r1 = theta * u1 / un, r2 = theta * u2 / un;
    const double ang = norm3(r0, r1, r2);
    double sc;
    if (ang <= 1e-3) {
        const double a2 = ang * ang;
        sc = 0.5 - a2 / 48 + a2 * a2 / 3840;
    } else {
        sc = sin(ang / 2) / ang;
    }
    const double x = sc * r0, y = sc * r1, z = sc * r2, w = cos(ang / 2);
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    const double R[9] = {x2 - y2 - z2 + w2, 2 * (xy - zw),      2 * (xz + yw),
                         2 * (xy + zw),      -x2 + y2 - z2 + w2, 2 * (yz - xw),
                         2 * (xz - yw),      2 * (yz + xw),      -x2 - y2 + z2 + w2};
    const double c0 = v[0], c1 = v[1], c2 = v[2];
    for (int i = 0; i < 9; ++i) {
        const double d0 = v[i * 3] - c0, d1 = v[i * 3 + 1] - c1, d2 = v[i * 3 + 2] - c2;
#pragma unroll
        for (int j = 0; j < 3; ++j) o[i * 3 + j] = d0 * R[j] + d1 * R[3 + j] + d2 * R[6 + j] + (j == 0 ? c0 : (j == 1 ? c1 : c2));
    }
}

// ---- viewpoint (eval_image_official.py:864-994) ----
// Solve A x = e3 (the last column of inv(A), what transform[:3, 3:] reads) by Gaussian elimination with partial pivoting
// -- LAPACK getrf's choice (first largest magnitude).  An exactly zero pivot is where numpy's inv raises and the reference
// falls back to pinv: returns false (the caller flags it rather than emulating pinv).
BOX_HD bool solve4_e3(double A[16], double x[4]) {
    double b[4] = {0., 0., 0., 1.};
    for (int k = 0; k < 4; ++k) {
        int p = k;
        double best = fabs(A[k * 4 + k]);
        for (int r = k + 1; r < 4; ++r)
            if (fabs(A[r * 4 + k]) > best) best = fabs(A[r * 4 + k]), p = r;
        if (!(best != 0.)) return false;
        if (p != k) {
            for (int c = 0; c < 4; ++c) {
                const double tmp = A[k * 4 + c];
                A[k * 4 + c] = A[p * 4 + c];
                A[p * 4 + c] = tmp;
            }
            const double tb = b[k];
            b[k] = b[p];
            b[p] = tb;
        }
        for (int r = k + 1; r < 4; ++r) {
            const double l = A[r * 4 + k] / A[k * 4 + k];
            for (int c = k + 1; c < 4; ++c) A[r * 4 + c] -= l * A[k * 4 + c];
            b[r] -= l * b[k];
        }
    }
    for (int k = 3; k >= 0; --k) {
        double s = b[k];
        for (int c = k + 1; c < 4; ++c) s -= A[k * 4 + c] * x[c];
        x[k] = s / A[k * 4 + k];
    }
    return true;
}

// compute_ray: the translation column of ((S' Vo)_h Vc'_h^T) (Vc'_h Vc'_h^T)^-1
BOX_HD bool compute_ray(const double* box, double ray[3]) {
    const double sz[3] = {norm3(box[15] - box[3], box[16] - box[4], box[17] - box[5]),
                          norm3(box[9] - box[3], box[10] - box[4], box[11] - box[5]),
                          norm3(box[6] - box[3], box[7] - box[4], box[8] - box[5])};
    double cct[16], oct[12];
    for (int a = 0; a < 4; ++a) {
        for (int b = 0; b < 4; ++b) {
            double s = 0.;
            for (int i = 0; i < 9; ++i) s += (a < 3 ? box[i * 3 + a] : 1.) * (b < 3 ? box[i * 3 + b] : 1.);
            cct[a * 4 + b] = s;
        }
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 4; ++b) {
            double s = 0.;
            for (int i = 0; i < 9; ++i) {
                const double unit = i == 0 ? 0. : ((((i - 1) >> (2 - a)) & 1) ? 0.5 : -0.5);  // Box.UNIT_BOX
                s += unit * sz[a] * (b < 3 ? box[i * 3 + b] : 1.);
            }
            oct[a * 4 + b] = s;
        }
    }
    double x[4];
    if (!solve4_e3(cct, x)) return false;
    for (int a = 0; a < 3; ++a) ray[a] = oct[a * 4] * x[0] + oct[a * 4 + 1] * x[1] + oct[a * 4 + 2] * x[2] + oct[a * 4 + 3] * x[3];
    return true;
}

// compute_viewpoint: azimuth atan2(z, x), elevation atan2(y, hypot(x, z)), in degrees (math.degrees: x * (180 / pi))
BOX_HD bool compute_viewpoint(const double* box, double& az, double& pol) {
    double r[3];
    if (!compute_ray(box, r)) return false;
    const double rad2deg = 180.0 / 3.141592653589793;
    az = atan2(r[2], r[0]) * rad2deg;
    pol = atan2(r[1], hypot(r[0], r[2])) * rad2deg;
    return true;
}

// evaluate_viewpoint: |polar difference|, |azimuth difference| % (360 / n) folded above 180.  A singular ray solve
// leaves both errors NaN and returns CP_BOX_FLAG_SINGULAR_RAY.
BOX_HD int evaluate_viewpoint(const double* box, const double* inst, int num_symmetry, double& az_err, double& pol_err) {
    double pa, pp, ga, gp;
    if (!compute_viewpoint(box, pa, pp) || !compute_viewpoint(inst, ga, gp)) {
        az_err = pol_err = NAN;
        return CP_BOX_FLAG_SINGULAR_RAY;
    }
    pol_err = fabs(pp - gp);
    double a = fmod(fabs(pa - ga), 360. / (double)num_symmetry);
    if (a > 180.) a = 360. - a;
    az_err = a;
    return 0;
}

// compute_average_distance: ADD, and ADD-S with the first minimum over ground-truth points (strict <, start at point 0)
BOX_HD void average_distance(const double* box, const double* inst, double& add, double& adds) {
    double s = 0.;
    for (int i = 0; i < 9; ++i)
        s += norm3(box[i * 3] - inst[i * 3], box[i * 3 + 1] - inst[i * 3 + 1], box[i * 3 + 2] - inst[i * 3 + 2]);
    add = s / 9.;
    double ss = 0.;
    for (int i = 0; i < 9; ++i) {
        double dmin = norm3(box[i * 3] - inst[0], box[i * 3 + 1] - inst[1], box[i * 3 + 2] - inst[2]);
        for (int j = 0; j < 9; ++j) {
            const double d = norm3(box[i * 3] - inst[j * 3], box[i * 3 + 1] - inst[j * 3 + 1], box[i * 3 + 2] - inst[j * 3 + 2]);
            if (d < dmin) dmin = d;
        }
        ss += dmin;
    }
    adds = ss / 9.;
}

// ---- evaluate_2d (eval_image_official.py:673-719) ----
// np.linalg.inv of a general 4 x 4 (Gauss-Jordan with partial pivoting); false where numpy raises
BOX_HD bool inv4(const double* M, double* out) {
    double A[16], I[16];
    for (int k = 0; k < 16; ++k) A[k] = M[k], I[k] = (k % 5 == 0) ? 1. : 0.;
    for (int k = 0; k < 4; ++k) {
        int p = k;
        double best = fabs(A[k * 4 + k]);
        for (int r = k + 1; r < 4; ++r)
            if (fabs(A[r * 4 + k]) > best) best = fabs(A[r * 4 + k]), p = r;
        if (!(best != 0.)) return false;
        if (p != k) {
            for (int c = 0; c < 4; ++c) {
                double tmp = A[k * 4 + c];
                A[k * 4 + c] = A[p * 4 + c];
                A[p * 4 + c] = tmp;
                tmp = I[k * 4 + c];
                I[k * 4 + c] = I[p * 4 + c];
                I[p * 4 + c] = tmp;
            }
        }
        const double piv = A[k * 4 + k];
        for (int c = 0; c < 4; ++c) A[k * 4 + c] /= piv, I[k * 4 + c] /= piv;
        for (int r = 0; r < 4; ++r) {
            if (r == k) continue;
            const double l = A[r * 4 + k];
            for (int c = 0; c < 4; ++c) A[r * 4 + c] -= l * A[k * 4 + c], I[r * 4 + c] -= l * I[k * 4 + c];
        }
    }
    for (int k = 0; k < 16; ++k) out[k] = I[k];
    return true;
}

BOX_HD void mul4(const double* A, const double* B, double* C) {
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            C[r * 4 + c] = A[r * 4] * B[c] + A[r * 4 + 1] * B[4 + c] + A[r * 4 + 2] * B[8 + c] + A[r * 4 + 3] * B[12 + c];
}

// One reprojection of the sweep: the ground truth rotated by theta about the object's y axis,
// proj @ Mo2c @ R_y(theta) @ Mc2o, perspective divide, viewport (p + 1) / 2 with x and y swapped, and the mean distance
// to the predicted 2D points over rows 1..8 (np.mean of 8: numpy's pairwise sum of 8 terms)
BOX_HD double reprojection_error(const double* pred2d, const double* inst3d, const double* proj, const double* mo2c,
                                 const double* mc2o, double theta) {
    const double c = cos(theta), s = sin(theta);
    const double MR[16] = {c, 0, s, 0, 0, 1, 0, 0, -s, 0, c, 0, 0, 0, 0, 1};
    double T1[16], T2[16], M[16];
    mul4(proj, mo2c, T1);
    mul4(T1, MR, T2);
    mul4(T2, mc2o, M);
    double e[8];
    for (int i = 1; i < 9; ++i) {
        const double X = inst3d[i * 3], Y = inst3d[i * 3 + 1], Z = inst3d[i * 3 + 2];
        const double q0 = M[0] * X + M[1] * Y + M[2] * Z + M[3];
        const double q1 = M[4] * X + M[5] * Y + M[6] * Z + M[7];
        const double q3 = M[12] * X + M[13] * Y + M[14] * Z + M[15];
        const double vx = (q0 / q3 + 1.0) / 2.0, vy = (q1 / q3 + 1.0) / 2.0;
        const double dx = pred2d[i * 2] - vy, dy = pred2d[i * 2 + 1] - vx;
        e[i - 1] = sqrt(dx * dx + dy * dy);
    }
    return (((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]))) / 8.;
}

// angle of 2D sweep index r: (2 pi / n) * r, no endpoint
BOX_HD double sweep_angle_2d(int r, int n) { return (TWO_PI / (double)n) * (double)r; }

// ---- per-rotation work of box_eval_kernel and of the host build ----
struct Best3 {
    double iou, add, adds, az, pol;
    int idx, flags;
};
struct Best2 {
    double err;
    int idx;
};

// the first maximum over rotation indices (the reference's sequential `iou > iou_best`, iou_best starting at 0)
BOX_HD bool better3(const Best3& a, const Best3& b) {
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    return a.iou > b.iou || (a.iou == b.iou && a.idx < b.idx);
}
// the first minimum (`error_best > error`, error_best starting at inf)
BOX_HD bool better2(const Best2& a, const Best2& b) {
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    return a.err < b.err || (a.err == b.err && a.idx < b.idx);
}

// rotation r of evaluate_3d: IoU of the rotated prediction and, where it beats `best`, ADD / ADD-S / viewpoint
BOX_HD void eval_rotation3(const double* pred, const double* gt, int r, int n, double* bufA, double* bufB, int st,
                           Best3& best, int& clip_flags) {
    double rot[27];
    rotate_box(pred, sweep_angle(r, n), rot);
    const double iou = box_iou(rot, gt, bufA, bufB, st, clip_flags);
    if (iou > (best.idx < 0 ? 0. : best.iou)) {
        best.iou = iou;
        best.idx = r;
        best.flags = evaluate_viewpoint(rot, gt, n, best.az, best.pol);
        average_distance(rot, gt, best.add, best.adds);
    }
}

BOX_HD void eval_rotation2(const double* pred2d, const double* gt, const double* proj, const double* mo2c,
                           const double* mc2o, int r, int n, Best2& best) {
    const double err = reprojection_error(pred2d, gt, proj, mo2c, mc2o, sweep_angle_2d(r, n));
    if ((best.idx < 0 ? INFINITY : best.err) > err) best.err = err, best.idx = r;
}

// the output record from the reduced bests: with no rotation of IoU > 0, ADD = ADD-S = _MAX_DISTANCE, IoU 0 and the
// viewpoint errors of the unrotated prediction (evaluate_3d computes those before its loop)
BOX_HD void write_record(const double* pred, const double* gt, int n, const Best3& b3, const Best2& b2, int clip_flags,
                         bool mo2c_ok, double* o) {
    int flags = clip_flags | (mo2c_ok ? 0 : CP_BOX_FLAG_SINGULAR_MO2C);
    if (b3.idx >= 0) {
        o[0] = b3.iou, o[1] = b3.add, o[2] = b3.adds, o[3] = b3.az, o[4] = b3.pol;
        flags |= b3.flags;
    } else {
        double az, pol;
        flags |= evaluate_viewpoint(pred, gt, n, az, pol);
        o[0] = 0., o[1] = MAX_DISTANCE, o[2] = MAX_DISTANCE, o[3] = az, o[4] = pol;
    }
    o[5] = b2.idx >= 0 ? b2.err : (mo2c_ok ? INFINITY : NAN);
    o[6] = (double)b3.idx;
    o[7] = (double)b2.idx;
    o[8] = (double)flags;
}

}  // namespace box3d

#if defined(__clang__)
#pragma clang fp contract(fast)  // hipcc's default again for whatever the including file defines after this header
#endif
