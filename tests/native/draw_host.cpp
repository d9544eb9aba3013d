// Host build of centerpose_amd/csrc/draw_common.h for tests/test_draw_cpu.py: the same source the device's overlay kernels
// run (the rule, the font, the per-record lists), driven primitive by primitive in order.
#include <cstddef>
#include <cstring>

#include "../../centerpose_amd/csrc/draw_common.h"

extern "C" {

// frames [B, H, pitch] uint8, prims [B, P, 8]: painter's order by drawing in order, only covered pixels written
void cp_draw_host_primitives(unsigned char* frames, int B, int H, int W, size_t pitch, const int* prims, int P) {
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < P; ++i) {
            const int* p = prims + ((size_t)b * P + i) * 8;
            int bb[4];
            if (!draw_prim_bbox(p, W, H, bb)) continue;
            for (int y = bb[1]; y <= bb[3]; ++y)
                for (int x = bb[0]; x <= bb[2]; ++x)
                    if (draw_covers(p, x, y)) {
                        unsigned char* q = frames + ((size_t)b * H + y) * pitch + (size_t)x * 3;
                        q[0] = (unsigned char)(p[6] & 0xFF);
                        q[1] = (unsigned char)((p[6] >> 8) & 0xFF);
                        q[2] = (unsigned char)((p[6] >> 16) & 0xFF);
                    }
        }
}

unsigned long long cp_draw_host_glyph(int code) { return draw_glyph_bits(code); }

int cp_draw_host_params_bytes(void) { return (int)sizeof(DrawParams); }

void cp_draw_host_cuboid_cam(const double* scale3, const double* loc, const double* quat, double* out27) {
    draw_cuboid_cam(scale3, loc, quat, out27);
}

// one record into its CP_DRAW_SLOTS slots; proj16 / box27 / cam4 may be null
void cp_draw_host_record(const void* params, double score, const double* bbox, const double* proj16, const double* box27,
                         const double* cam4, double id, int* slots) {
    DrawParams P;
    std::memcpy(&P, params, sizeof(P));
    draw_build_record(P, score, bbox, proj16, box27, cam4, id, slots);
}
}
