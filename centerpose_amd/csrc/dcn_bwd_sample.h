// The DCNv2 backward's sample (dcn_bwd.hip's data and weight-gradient kernels, dcn_bwd16.hip's column kernel): written once, so
// that the materialised columns of the f16x3 mode are the values the float32 weight gradient builds in its lanes.
#pragma once
#include <hip/hip_runtime.h>

// One sample: position, 1-D weights and corner validity (dcn_v2_im2col_cuda.cu dmcn_im2col_bilinear / the get_*_weight
// helpers use the same floor / +1 corners and the same in-image tests).
struct Sample {
    bool in;          // inside (-1, H) x (-1, W): otherwise it contributes to nothing
    int y0, x0;       // low corner
    float lh, lw, hh, hw;
    bool c1, c2, c3, c4;  // (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1) inside the image
};

__device__ __forceinline__ Sample make_sample(float sy, float sx, int H, int W) {
    Sample s;
    s.in = !(sy <= -1.f || sx <= -1.f || sy >= (float)H || sx >= (float)W);
    const float fy = floorf(sy), fx = floorf(sx);
    // `in` is true for a NaN coordinate (every comparison above is false): the sample's weights are NaN and so is everything it
    // contributes to.  Its corner is (0, 0) by statement (fy == fy), not by what a float-to-int conversion makes of a NaN: for a
    // finite coordinate `in` bounds y0 to [-1, H - 1] and x0 to [-1, W - 1], for a NaN one they are 0, and c1 .. c4 below then
    // keep every corner that is read or written inside the image.
    s.y0 = s.in ? (fy == fy ? (int)fy : 0) : -2;
    s.x0 = s.in ? (fx == fx ? (int)fx : 0) : -2;
    s.lh = sy - fy;
    s.lw = sx - fx;
    s.hh = 1.f - s.lh;
    s.hw = 1.f - s.lw;
    s.c1 = s.in && s.y0 >= 0 && s.x0 >= 0;
    s.c2 = s.in && s.y0 >= 0 && s.x0 + 1 <= W - 1;
    s.c3 = s.in && s.y0 + 1 <= H - 1 && s.x0 >= 0;
    s.c4 = s.in && s.y0 + 1 <= H - 1 && s.x0 + 1 <= W - 1;
    return s;
}
