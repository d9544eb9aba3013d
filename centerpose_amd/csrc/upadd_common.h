// IDAUp's depth-wise ConvTranspose2d(C, C, k = 2f, stride = f, padding = f/2, groups = C) + add (pose_dla_dcn.py:411-417), the
// arithmetic of one 16-byte piece (4 channels of one output pixel).  Shared by the stand-alone kernel (ewise.hip:
// upsample_add_kernel) and by the DCN epilogue that writes node(u) + up(t) in place of the node's own output (dcn16t.hip), so
// that both forms multiply, contract and round identically.
//   out[y,x,c] = add[y,x,c] + sum_{ky,kx} in[(y+p-ky)/f, (x+p-kx)/f, c] * w[c,ky,kx],  p = f/2,
// over the taps with (y+p-ky) % f == 0: exactly two per axis.
#pragma once
#include <hip/hip_runtime.h>

// One axis: output coordinate y -> its first kernel tap k0 = (y+p) % f and that tap's source coordinate i0.  The second tap is
// k0 + f, read from i0 - 1.  Sources outside [0, n) do not exist (the caller supplies zeros for them).
__device__ __forceinline__ void cp_upadd_axis(int y, int f, int* k0, int* i0) {
    const int p = f / 2;
    *k0 = (y + p) % f;
    *i0 = (y + p - *k0) / f;
}

// v[a][bb]: the source at (iy0 - a, ix0 - bb), zeros where it does not exist; w[a][bb]: the weights of tap (ky0 + a f, kx0 + bb f).
// The four taps are summed in (a, bb) order starting from s = 0, then add + s.
__device__ __forceinline__ float4 cp_upadd_piece(const float4 (&v)[2][2], const float4 (&w)[2][2], float4 add) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            s.x += v[a][bb].x * w[a][bb].x;
            s.y += v[a][bb].y * w[a][bb].y;
            s.z += v[a][bb].z * w[a][bb].z;
            s.w += v[a][bb].w * w[a][bb].w;
        }
    add.x += s.x; add.y += s.y; add.z += s.z; add.w += s.w;
    return add;
}
