// The overlay's rasterising rule and the per-record primitive lists, as plain scalar functions that compile for the device
// (draw.hip) and for the host (tests/native/draw_host.cpp builds the very same functions with g++; tests/draw_ref.py is the
// numpy restatement both are compared with, bit for bit).
//
// A primitive is 8 x int32: kind, x0, y0, x1, y1, size, colour (B | G << 8 | R << 16), aux.  The rule is this project's own
// (cv2 is not available to pin its thick-line code to): exact, in integers, independent of launch shape and tiling.
//   kind 1  segment          size = thickness t in 1..16; covered iff 4 dist^2(Q, segment P0P1) <= t^2 (a capsule)
//   kind 2  disc             size = radius r in 0..64; covered iff |Q - P0|^2 <= r^2
//   kind 3  rectangle        size = thickness t; the union of the four segments between (x0,y0) (x1,y0) (x1,y1) (x0,y1)
//   kind 4  filled rectangle both corners inclusive, corners in any order
//   kind 5  glyph            aux = ASCII code, (x0, y0) = top-left of the cell, size = integer scale s in 1..8; every set bit of
//                            the 5 x 7 bitmap is an s x s block (cell pitch 6 s: text layout is the caller's)
//   anything else            nothing
// Every coordinate lies in [-8192, 8191] and frames are at most 8192 x 8192; a primitive with a coordinate or a size outside
// its range is skipped whole, never clamped (this also covers the reference's <= -10000 "no such vertex" sentinel).
//
// Bounds: with Q in [0, 8191]^2 and P in [-8192, 8191]^2 every component of w = Q - P0 and d = P1 - P0 is below 2^14 in
// magnitude, so s = w.d, L2 = d.d and cross(w, d) are below 2^29 (int32), 4 |w|^2 <= 8 * 16383^2 < 2^31 (int32, just),
// 4 cross^2 < 2^60 and t^2 L2 < 2^37 (int64).
#pragma once
#include <math.h>
#include <stdint.h>

// no fused multiply-adds: the axes' float64 arithmetic restates numpy expressions whose every operation rounds
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#ifdef __HIPCC__
#define DRAW_HD __host__ __device__ __forceinline__
#else
#define DRAW_HD static inline
#endif

// (repeated from include/centerpose_hip.h so that the host build needs no other header; a drifting copy is a compile error)
#define CP_DRAW_SEGMENT 1
#define CP_DRAW_DISC 2
#define CP_DRAW_RECT 3
#define CP_DRAW_FILL 4
#define CP_DRAW_GLYPH 5
#define CP_DRAW_COORD_MIN (-8192)
#define CP_DRAW_COORD_MAX 8191
#define CP_DRAW_MAX_DIM 8192
#define CP_DRAW_MAX_P 65536
#define CP_DRAW_SLOTS 44
#define CP_DRAW_SLOT_BOX 0
#define CP_DRAW_SLOT_LABEL 1   /* the label's filled rectangle, then CP_DRAW_LABEL_CHARS glyphs */
#define CP_DRAW_LABEL_CHARS 13 /* "ID:" + at most 10 digits */
#define CP_DRAW_SLOT_DISCS 15  /* 8 vertices */
#define CP_DRAW_SLOT_EDGES 23  /* 12 edges */
#define CP_DRAW_SLOT_CROSS 35  /* front, top, top, front, top, top: the reference's nested loop as it runs */
#define CP_DRAW_SLOT_AXES 41   /* y, z, x */
#define CP_DRAW_LABEL_SCALE 2
// the reference's colour of category 0 (utils/debugger.py: color_list[0] through the theme arithmetic of __init__ and
// add_coco_bbox), computed once when tests/golden/draw_calls.json was recorded
#define CP_DRAW_CAT0_BLACK 0xFFFFFF /* theme 'black': (255, 255, 255) */
#define CP_DRAW_CAT0_WHITE 0x8080FF /* theme 'white': B 255, G 128, R 128 */

struct DrawParams {  // cp_draw_params of include/centerpose_hip.h, field for field
    double vis_thresh;
    int reg_bbox, show_axes, paper_display, tracking_task, theme, labels, width, height;
};

// ---- the font: 5 x 7 bitmaps of this project (row r, column c at bit 5 r + 4 - c); 0 = the code draws nothing ----
#define DRAW_G(a, b, c, d, e, f, g)                                                                                         \
    ((uint64_t)(a) | (uint64_t)(b) << 5 | (uint64_t)(c) << 10 | (uint64_t)(d) << 15 | (uint64_t)(e) << 20 | (uint64_t)(f) << 25 | \
     (uint64_t)(g) << 30)
DRAW_HD uint64_t draw_glyph_bits(int code) {
    switch (code) {
        case '0': return DRAW_G(0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110);
        case '1': return DRAW_G(0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110);
        case '2': return DRAW_G(0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111);
        case '3': return DRAW_G(0b11111, 0b00010, 0b00100, 0b00010, 0b00001, 0b10001, 0b01110);
        case '4': return DRAW_G(0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010);
        case '5': return DRAW_G(0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110);
        case '6': return DRAW_G(0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110);
        case '7': return DRAW_G(0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000);
        case '8': return DRAW_G(0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110);
        case '9': return DRAW_G(0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100);
        case '.': return DRAW_G(0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b01100, 0b01100);
        case ':': return DRAW_G(0b00000, 0b01100, 0b01100, 0b00000, 0b01100, 0b01100, 0b00000);
        case '/': return DRAW_G(0b00001, 0b00001, 0b00010, 0b00100, 0b01000, 0b10000, 0b10000);
        case '-': return DRAW_G(0b00000, 0b00000, 0b00000, 0b11111, 0b00000, 0b00000, 0b00000);
        case 'o': return DRAW_G(0b00000, 0b00000, 0b01110, 0b10001, 0b10001, 0b10001, 0b01110);
        case 'p': return DRAW_G(0b00000, 0b00000, 0b11110, 0b10001, 0b11110, 0b10000, 0b10000);
        case 'I': return DRAW_G(0b01110, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110);
        case 'D': return DRAW_G(0b11100, 0b10010, 0b10001, 0b10001, 0b10001, 0b10010, 0b11100);
        case 'P': return DRAW_G(0b11110, 0b10001, 0b10001, 0b11110, 0b10000, 0b10000, 0b10000);
        case 'r': return DRAW_G(0b00000, 0b00000, 0b10110, 0b11001, 0b10000, 0b10000, 0b10000);
        case 'e': return DRAW_G(0b00000, 0b00000, 0b01110, 0b10001, 0b11111, 0b10000, 0b01110);
        case 'd': return DRAW_G(0b00001, 0b00001, 0b01101, 0b10011, 0b10001, 0b10001, 0b01111);
        case 'F': return DRAW_G(0b11111, 0b10000, 0b10000, 0b11110, 0b10000, 0b10000, 0b10000);
        case 'a': return DRAW_G(0b00000, 0b00000, 0b01110, 0b00001, 0b01111, 0b10001, 0b01111);
        case 'm': return DRAW_G(0b00000, 0b00000, 0b11010, 0b10101, 0b10101, 0b10001, 0b10001);
        case 'G': return DRAW_G(0b01110, 0b10001, 0b10000, 0b10111, 0b10001, 0b10001, 0b01111);
        case 'T': return DRAW_G(0b11111, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100, 0b00100);
        case 'n': return DRAW_G(0b00000, 0b00000, 0b10110, 0b11001, 0b10001, 0b10001, 0b10001);
        default: return 0;  // (the space among them: it only advances the pen)
    }
}

// ---- the rule ----
DRAW_HD bool draw_coord_ok(int v) { return v >= CP_DRAW_COORD_MIN && v <= CP_DRAW_COORD_MAX; }
DRAW_HD int draw_min(int a, int b) { return a < b ? a : b; }
DRAW_HD int draw_max(int a, int b) { return a > b ? a : b; }

// A primitive that draws at all on a W x H frame: its kind is known, its coordinates and size are in range and its bounding
// box meets the frame.  bb = that box clipped to the frame, inclusive (x0, y0, x1, y1); it may be generous, never tight.
DRAW_HD bool draw_prim_bbox(const int* p, int W, int H, int* bb) {
    const int kind = p[0], x0 = p[1], y0 = p[2], x1 = p[3], y1 = p[4], size = p[5];
    if (!draw_coord_ok(x0) || !draw_coord_ok(y0) || !draw_coord_ok(x1) || !draw_coord_ok(y1)) return false;
    int lx, ly, hx, hy;
    if (kind == CP_DRAW_SEGMENT || kind == CP_DRAW_RECT) {
        if (size < 1 || size > 16) return false;
        const int m = (size + 1) / 2;
        lx = draw_min(x0, x1) - m; hx = draw_max(x0, x1) + m;
        ly = draw_min(y0, y1) - m; hy = draw_max(y0, y1) + m;
    } else if (kind == CP_DRAW_DISC) {
        if (size < 0 || size > 64) return false;
        lx = x0 - size; hx = x0 + size; ly = y0 - size; hy = y0 + size;
    } else if (kind == CP_DRAW_FILL) {
        lx = draw_min(x0, x1); hx = draw_max(x0, x1); ly = draw_min(y0, y1); hy = draw_max(y0, y1);
    } else if (kind == CP_DRAW_GLYPH) {
        if (size < 1 || size > 8 || draw_glyph_bits(p[7]) == 0) return false;
        lx = x0; hx = x0 + 5 * size - 1; ly = y0; hy = y0 + 7 * size - 1;
    } else {
        return false;
    }
    if (hx < 0 || hy < 0 || lx >= W || ly >= H) return false;
    bb[0] = draw_max(lx, 0); bb[1] = draw_max(ly, 0); bb[2] = draw_min(hx, W - 1); bb[3] = draw_min(hy, H - 1);
    return true;
}

// 4 dist^2((x, y), segment (x0,y0)-(x1,y1)) <= t^2, exactly (the bounds argument is at the top of this file)
DRAW_HD bool draw_seg_covers(int x0, int y0, int x1, int y1, int t, int x, int y) {
    const int dx = x1 - x0, dy = y1 - y0, wx = x - x0, wy = y - y0;
    const int L2 = dx * dx + dy * dy, s = wx * dx + wy * dy, t2 = t * t;
    if (L2 == 0 || s <= 0) return 4 * (wx * wx + wy * wy) <= t2;
    if (s >= L2) {
        const int ex = x - x1, ey = y - y1;
        return 4 * (ex * ex + ey * ey) <= t2;
    }
    const int64_t cr = (int64_t)(wx * dy - wy * dx);
    return 4 * cr * cr <= (int64_t)t2 * L2;
}

// whether the primitive p (one that draw_prim_bbox accepted) covers the pixel (x, y)
DRAW_HD bool draw_covers(const int* p, int x, int y) {
    const int kind = p[0], x0 = p[1], y0 = p[2], x1 = p[3], y1 = p[4], size = p[5];
    if (kind == CP_DRAW_SEGMENT) return draw_seg_covers(x0, y0, x1, y1, size, x, y);
    if (kind == CP_DRAW_DISC) {
        const int wx = x - x0, wy = y - y0;
        return wx * wx + wy * wy <= size * size;
    }
    if (kind == CP_DRAW_RECT)
        return draw_seg_covers(x0, y0, x1, y0, size, x, y) || draw_seg_covers(x1, y0, x1, y1, size, x, y) ||
               draw_seg_covers(x1, y1, x0, y1, size, x, y) || draw_seg_covers(x0, y1, x0, y0, size, x, y);
    if (kind == CP_DRAW_FILL)
        return x >= draw_min(x0, x1) && x <= draw_max(x0, x1) && y >= draw_min(y0, y1) && y <= draw_max(y0, y1);
    if (kind == CP_DRAW_GLYPH) {
        const int gx = x - x0, gy = y - y0;
        if (gx < 0 || gy < 0 || gx >= 5 * size || gy >= 7 * size) return false;
        return (draw_glyph_bits(p[7]) >> (5 * (gy / size) + 4 - gx / size)) & 1;
    }
    return false;
}

// ---- the lists: what the reference draws per record (detectors/object_pose.py:357-392 `save_results` through
// utils/debugger.py:131-162 `add_coco_bbox`, :214-296 `add_coco_hp`, :299-320 `add_axes`), into the record's fixed slots ----

// a float64 coordinate as the reference's np.int32 cast / int() takes it (towards zero); false when it is not finite or leaves
// the coordinate range: the primitive that needs it is withdrawn
DRAW_HD bool draw_trunc(double v, int* out) {
    if (!(fabs(v) < 8193.0)) return false;
    const int i = (int)v;
    *out = i;
    return draw_coord_ok(i);
}

DRAW_HD void draw_emit(int* slot, int kind, int x0, int y0, int x1, int y1, int size, int colour, int aux) {
    slot[0] = kind; slot[1] = x0; slot[2] = y0; slot[3] = x1; slot[4] = y1; slot[5] = size; slot[6] = colour; slot[7] = aux;
}

// the camera-frame cuboid of `finish_detection` (utils/pnp/cuboid_pnp_shell.py:26-51): centroid first, then the 8 vertices of
// the box of size scale / scale_y posed by (quaternion xyzw, location)
DRAW_HD void draw_cuboid_cam(const double* scale3, const double* loc, const double* q, double* out27) {
    const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double x = q[0] / n, y = q[1] / n, z = q[2] / n, w = q[3] / n;
    const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w),     2 * (x * z + y * w),
                         2 * (x * y + z * w),     1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w),     2 * (y * z + x * w),     1 - 2 * (x * x + y * y)};
    const double sw = scale3[0] / scale3[1], sh = 1.0, sd = scale3[2] / scale3[1];
    double cm[3] = {0, 0, 0};
    for (int v = 0; v < 8; ++v) {
        const double vx = (v & 4) ? sw / 2 : -sw / 2, vy = (v & 2) ? sh / 2 : -sh / 2, vz = (v & 1) ? sd / 2 : -sd / 2;
        for (int r = 0; r < 3; ++r) {
            const double c = R[3 * r] * vx + R[3 * r + 1] * vy + R[3 * r + 2] * vz + loc[r];
            out27[3 * (v + 1) + r] = c;
            cm[r] += c;
        }
    }
    for (int r = 0; r < 3; ++r) out27[r] = cm[r] / 8;
}

// One record into its CP_DRAW_SLOTS slots (every slot it does not use is left all zero, kind 0).
//   bbox [4], proj16 (projected_cuboid, or null: no cuboid), box27 (the 9 x 3 camera-frame box add_axes reads, or null),
//   cam4 (fx, fy, cx, cy, or null), id (the tracking id; drawn with P.labels and P.tracking_task only)
DRAW_HD void draw_build_record(const DrawParams& P, double score, const double* bbox, const double* proj16, const double* box27,
                               const double* cam4, double id, int* slots) {
    for (int i = 0; i < CP_DRAW_SLOTS * 8; ++i) slots[i] = 0;
    if (!(score > P.vis_thresh) || !P.reg_bbox) return;
    const int cat0 = P.theme ? CP_DRAW_CAT0_WHITE : CP_DRAW_CAT0_BLACK;
    if (!P.paper_display) {
        int b[4];
        if (draw_trunc(bbox[0], &b[0]) && draw_trunc(bbox[1], &b[1]) && draw_trunc(bbox[2], &b[2]) && draw_trunc(bbox[3], &b[3])) {
            b[0] = draw_min(draw_max(b[0], 0), P.width);
            b[1] = draw_min(draw_max(b[1], 0), P.height);
            b[2] = draw_min(draw_max(b[2], 0), P.width);
            b[3] = draw_min(draw_max(b[3], 0), P.height);
            draw_emit(slots + 8 * CP_DRAW_SLOT_BOX, CP_DRAW_RECT, b[0], b[1], b[2], b[3], 2, cat0, 0);
            if (P.labels && P.tracking_task && id >= 0 && id < 1e10) {
                // "ID:<n>" on a filled rectangle above the box (add_coco_bbox's geometry with this font's text size)
                int txt[CP_DRAW_LABEL_CHARS], n = 0;
                txt[n++] = 'I'; txt[n++] = 'D'; txt[n++] = ':';
                long long v = (long long)id;
                int digits[10], nd = 0;
                do { digits[nd++] = (int)(v % 10); v /= 10; } while (v > 0 && nd < 10);
                while (nd > 0) txt[n++] = '0' + digits[--nd];
                const int s = CP_DRAW_LABEL_SCALE, tw = 6 * s * n - s, th = 7 * s;
                const int top = b[1] - th - 2;
                if (draw_coord_ok(top) && draw_coord_ok(b[0] + 6 * s * n)) {
                    draw_emit(slots + 8 * CP_DRAW_SLOT_LABEL, CP_DRAW_FILL, b[0], top, b[0] + tw, b[1] - 2, 0, cat0, 0);
                    for (int i = 0; i < n; ++i)
                        draw_emit(slots + 8 * (CP_DRAW_SLOT_LABEL + 1 + i), CP_DRAW_GLYPH, b[0] + 6 * s * i, top, 0, 0, s, 0x000000,
                                  txt[i]);
                }
            }
        }
    }
    if (!proj16) return;
    int px[8], py[8];
    bool ok[8];
    for (int j = 0; j < 8; ++j) ok[j] = draw_trunc(proj16[2 * j], &px[j]) && draw_trunc(proj16[2 * j + 1], &py[j]);
    const int hp[8] = {0xFF0000, 0xFFA500, 0xFFFF00, 0x008000, 0x0000FF, 0x4B0082, 0xEE82EE, 0x000000};  // colors_hp as R<<16|G<<8|B
    for (int j = 0; j < 8; ++j)
        if (ok[j])
            draw_emit(slots + 8 * (CP_DRAW_SLOT_DISCS + j), CP_DRAW_DISC, px[j], py[j], 0, 0, P.paper_display ? 10 : 5,
                      P.paper_display ? 0x00FFFF : hp[j], 0);
    const int edges[12][2] = {{1, 3}, {1, 5}, {5, 7}, {3, 7}, {0, 1}, {2, 3}, {4, 5}, {6, 7}, {0, 2}, {0, 4}, {2, 6}, {4, 6}};
    for (int e = 0; e < 12; ++e) {
        const int a = edges[e][0], c = edges[e][1];
        if (ok[a] && ok[c]) draw_emit(slots + 8 * (CP_DRAW_SLOT_EDGES + e), CP_DRAW_SEGMENT, px[a], py[a], px[c], py[c], 2, 0xFF0000, 0);
    }
    if (!P.paper_display) {
        // front cross, then the top cross inside the same loop, as the reference's indentation has it (drawn as plain segments)
        const int cross[6][2] = {{1, 7}, {2, 7}, {3, 6}, {3, 5}, {2, 7}, {3, 6}};
        for (int e = 0; e < 6; ++e) {
            const int a = cross[e][0], c = cross[e][1];
            if (ok[a] && ok[c])
                draw_emit(slots + 8 * (CP_DRAW_SLOT_CROSS + e), CP_DRAW_SEGMENT, px[a], py[a], px[c], py[c], 2, 0x000000, 0);
        }
    }
    if ((P.show_axes || P.paper_display) && box27 && cam4) {
        // add_axes: centroid, then 0.5 along the normalised top / front / right directions, projected, int()
        const int ends[3] = {3, 2, 5};
        int ax[4], ay[4];
        bool aok[4];
        for (int i = 0; i < 4; ++i) {
            double v[3] = {0, 0, 0};
            if (i > 0) {
                for (int r = 0; r < 3; ++r) v[r] = box27[3 * ends[i - 1] + r] - box27[3 + r];
                const double nrm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                for (int r = 0; r < 3; ++r) v[r] = nrm != 0 ? v[r] / nrm * 0.5 : 0.0;
            }
            for (int r = 0; r < 3; ++r) v[r] = v[r] + box27[r];
            const double u = (cam4[0] * v[0] + 0.0 * v[1] + cam4[2] * v[2]) / v[2];
            const double w = (0.0 * v[0] + cam4[1] * v[1] + cam4[3] * v[2]) / v[2];
            aok[i] = draw_trunc(u, &ax[i]) && draw_trunc(w, &ay[i]);
        }
        const int colour[3] = {0x00FF00, 0x0000FF, 0xFF0000};  // y green, z blue, x red (BGR tuples (0,255,0) (255,0,0) (0,0,255))
        for (int i = 0; i < 3; ++i)
            if (aok[0] && aok[i + 1])
                draw_emit(slots + 8 * (CP_DRAW_SLOT_AXES + i), CP_DRAW_SEGMENT, ax[0], ay[0], ax[i + 1], ay[i + 1], 5, colour[i], 0);
    }
}

#if defined(__clang__) && defined(__HIPCC__)
#pragma clang fp contract(fast)  // hipcc's default again for whatever the including file defines after this header
#endif
