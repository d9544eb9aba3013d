// What the deterministic DCNv2 input gradient (cp_dcnv2_backward_det, dcn_bwd.hip) computes per (pixel, tap, corner): the
// bilinear set-up of one sample, the entry id and the sort key "destination cell within the chunk of images".  Plain scalar
// code that also compiles for the host (tests/native/dcn_det_host.cpp), because the conversion of a sample position to a
// cell is the one place that path can index out of range.
//
// Fast geometry only: 3x3, stride 1, pad 1, dilation 1, one deformable group; H = Ho, W = Wo.
//   entry id  = ((pp * 9 + tap) * 4 + q),  pp = bi * H * W + pix  (bi: image within the chunk, pix = ho * W + wo)
//   key       = (bi * H + y) * W + x  for a corner (y, x) that contributes,  `cells` = nb * H * W  (the sentinel) otherwise
//   corner q  = 0: (y0, x0)  1: (y0, x0 + 1)  2: (y0 + 1, x0)  3: (y0 + 1, x0 + 1)
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define CP_DET_HD __host__ __device__ __forceinline__
#else
#define CP_DET_HD static inline
#endif

constexpr int DCN_DET_CHUNK = 512;  // a destination's list is summed in consecutive chunks of this many entries

// One sample, as dcn_bwd.hip's make_sample has it (the reference's dmcn_im2col_bilinear / get_*_weight corners and in-image
// tests).  A NaN position passes the reference's `<=` / `>=` tests; its low corner is then (0, 0) -- what the device's
// float-to-int conversion gives make_sample -- so that every integer here is defined on the host as well.  Where `in` holds
// and the position is a number, floor(s) lies in [-1, H - 1]: no conversion can overflow.
struct DcnDetSample {
    bool in;          // not outside (-1, H) x (-1, W): otherwise it contributes to nothing
    int y0, x0;       // low corner
    float lh, lw, hh, hw;
    bool c[4];        // corner q inside the image
};

CP_DET_HD DcnDetSample dcn_det_sample(float sy, float sx, int H, int W) {
    DcnDetSample s;
    s.in = !(sy <= -1.f || sx <= -1.f || sy >= (float)H || sx >= (float)W);
    const float fy = floorf(sy), fx = floorf(sx);
    s.y0 = s.in ? (fy == fy ? (int)fy : 0) : -2;
    s.x0 = s.in ? (fx == fx ? (int)fx : 0) : -2;
    s.lh = sy - fy;
    s.lw = sx - fx;
    s.hh = 1.f - s.lh;
    s.hw = 1.f - s.lw;
    s.c[0] = s.in && s.y0 >= 0 && s.x0 >= 0;
    s.c[1] = s.in && s.y0 >= 0 && s.x0 + 1 <= W - 1;
    s.c[2] = s.in && s.y0 + 1 <= H - 1 && s.x0 >= 0;
    s.c[3] = s.in && s.y0 + 1 <= H - 1 && s.x0 + 1 <= W - 1;
    return s;  // `in` bounds y0 to [-1, H - 1] and x0 to [-1, W - 1], so a set flag means 0 <= y < H and 0 <= x < W
}

// The sample of (pixel (ho, wo), tap) under offsets (oh, ow)
CP_DET_HD DcnDetSample dcn_det_sample_at(int ho, int wo, int tap, float oh, float ow, int H, int W) {
    const int i = tap / 3, j = tap - 3 * i;
    return dcn_det_sample((float)(ho - 1 + i) + oh, (float)(wo - 1 + j) + ow, H, W);
}

CP_DET_HD float dcn_det_weight(const DcnDetSample& s, int q) {
    return ((q & 2) ? s.lh : s.hh) * ((q & 1) ? s.lw : s.hw);
}

CP_DET_HD uint32_t dcn_det_id(uint32_t pp, int tap, int q) { return (pp * 9u + (uint32_t)tap) * 4u + (uint32_t)q; }

CP_DET_HD void dcn_det_decode(uint32_t id, uint32_t* pp, int* tap, int* q) {
    *q = (int)(id & 3u);
    const uint32_t r = id >> 2;
    *pp = r / 9u;
    *tap = (int)(r - *pp * 9u);
}

// Key of corner q: always in [0, cells]
CP_DET_HD uint32_t dcn_det_key(const DcnDetSample& s, int q, int bi, int H, int W, uint32_t cells) {
    if (!s.c[q]) return cells;
    const int y = s.y0 + (q >> 1), x = s.x0 + (q & 1);
    const uint32_t key = ((uint32_t)bi * (uint32_t)H + (uint32_t)y) * (uint32_t)W + (uint32_t)x;
    return key < cells ? key : cells;
}

// Radix passes of 8 bits that cover the keys 0 .. cells
CP_DET_HD int dcn_det_passes(uint32_t cells) {
    int bits = 1;
    while (bits < 32 && (cells >> bits) != 0) ++bits;
    return (bits + 7) / 8;
}
