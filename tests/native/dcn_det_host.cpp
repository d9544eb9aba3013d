// Host build of centerpose_amd/csrc/dcn_bwd_det_common.h for tests/test_dcn_backward_det_cpu.py: the id encode / decode, the
// sample -> key conversion, and the index build + stable LSD radix sort of dcn_bwd.hip restated with the same functions.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../centerpose_amd/csrc/dcn_bwd_det_common.h"

// ids 0 .. n-1: decode, re-encode, count the ones that do not come back (or decode out of range)
extern "C" uint32_t dcn_det_host_roundtrip(uint32_t n) {
    uint32_t bad = 0;
    for (uint32_t id = 0; id < n; ++id) {
        uint32_t pp;
        int tap, q;
        dcn_det_decode(id, &pp, &tap, &q);
        if (tap < 0 || tap > 8 || q < 0 || q > 3 || dcn_det_id(pp, tap, q) != id) ++bad;
    }
    return bad;
}

// n samples at positions (sy[i], sx[i]) of image bi: keys[i][4], valid[i][4] (the corner flags), in[i]
extern "C" void dcn_det_host_keys(const float* sy, const float* sx, int n, int bi, int H, int W, uint32_t cells, uint32_t* keys,
                                  int* valid, int* in) {
    for (int i = 0; i < n; ++i) {
        const DcnDetSample s = dcn_det_sample(sy[i], sx[i], H, W);
        in[i] = s.in;
        for (int q = 0; q < 4; ++q) {
            keys[4 * i + q] = dcn_det_key(s, q, bi, H, W, cells);
            valid[4 * i + q] = s.c[q];
        }
    }
}

extern "C" int dcn_det_host_passes(uint32_t cells) { return dcn_det_passes(cells); }

// offset [nb][18][H][W] -> the sorted (key, id) of all nb * H * W * 36 entries; returns the number of radix passes
extern "C" int dcn_det_host_index(const float* off, int nb, int H, int W, uint32_t* keys, uint32_t* ids) {
    const int HW = H * W;
    const uint32_t cells = (uint32_t)nb * HW, n = cells * 36u;
    std::vector<uint32_t> k0(n), i0(n), k1(n), i1(n);
    for (uint32_t e = 0; e < cells * 9u; ++e) {
        const uint32_t pp = e / 9u;
        const int tap = (int)(e - pp * 9u), bi = (int)(pp / (uint32_t)HW), pix = (int)(pp - (uint32_t)bi * HW);
        const int ho = pix / W, wo = pix - ho * W;
        const float oh = off[((size_t)bi * 18 + 2 * tap) * HW + pix], ow = off[((size_t)bi * 18 + 2 * tap + 1) * HW + pix];
        const DcnDetSample s = dcn_det_sample_at(ho, wo, tap, oh, ow, H, W);
        for (int q = 0; q < 4; ++q) {
            k0[4 * e + q] = dcn_det_key(s, q, bi, H, W, cells);
            i0[4 * e + q] = dcn_det_id(pp, tap, q);
        }
    }
    const int passes = dcn_det_passes(cells);
    for (int pass = 0; pass < passes; ++pass) {
        size_t start[257] = {0};
        for (uint32_t e = 0; e < n; ++e) ++start[((k0[e] >> (8 * pass)) & 255u) + 1];
        for (int d = 0; d < 256; ++d) start[d + 1] += start[d];
        for (uint32_t e = 0; e < n; ++e) {
            const size_t to = start[(k0[e] >> (8 * pass)) & 255u]++;
            k1[to] = k0[e];
            i1[to] = i0[e];
        }
        k0.swap(k1);
        i0.swap(i1);
    }
    for (uint32_t e = 0; e < n; ++e) keys[e] = k0[e], ids[e] = i0[e];
    return passes;
}
