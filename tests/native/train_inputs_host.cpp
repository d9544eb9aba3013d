// Host build of centerpose_amd/csrc/train_inputs_common.h for tests/test_train_inputs_cpu.py and
// tests/test_train_inputs_gpu.py: one image of cp_train_inputs, pixel by pixel, on the host.
#include "../../centerpose_amd/csrc/train_inputs_common.h"

using namespace train_inputs;

// frames: the packed frames buffer; rec: the image's record [CP_TI_STRIDE]; out: [3][OH][OW] float32.
// use_mean != 0: gs_mean is taken from *gs_mean (the device's own); else it is float32(sum / (OH OW)) of a float64 sum
// in pixel order, written back to *gs_mean (0 for an image without colour).
extern "C" void ti_host_image(const unsigned char* frames, const double* rec, const float* mean3, const float* std3, int OH,
                              int OW, int use_mean, float* gs_mean, float* out) {
    TiImage im;
    ti_decode(rec, &im);
    const unsigned char* img = frames + im.offset;
    float m = use_mean ? *gs_mean : 0.f;
    if (im.color && !use_mean) {
        double sum = 0.0;
        for (int y = 0; y < OH; ++y)
            for (int x = 0; x < OW; ++x) {
                float v[3];
                sum += (double)ti_pixel(img, &im, x, y, v);
            }
        m = (float)(sum / ((double)OH * OW));
    }
    if (!im.color) m = 0.f;
    *gs_mean = m;
    for (int y = 0; y < OH; ++y)
        for (int x = 0; x < OW; ++x) {
            float v[3];
            const float gs = ti_pixel(img, &im, x, y, v);
            if (im.color) ti_color(v, gs, m, &im);
            for (int c = 0; c < 3; ++c) out[((size_t)c * OH + y) * OW + x] = ti_normalise(v[c], mean3[c], std3[c]);
        }
}

extern "C" int ti_host_order_op(int order, int i) { return ti_order_op(order, i); }
