// The convolution kernel selectors of libcenterpose_hip.so (cp_conv_variant, cp_conv16_variant and the predicates beside them in
// centerpose_amd/csrc/cp_common.h) asked row by row by tests/test_conv_select_cpu.py and tools/make_conv_select_golden.py.  They are
// pure host functions of a ConvParams: nothing is launched and no HIP call is made.  Tensor pointers are null or a dummy that is
// never dereferenced, as in the engine's own dry plan; the weights' shapes follow the engine's packer (engine_pack.hip).
#include "../../centerpose_amd/csrc/cp_common.h"

#include <cstring>

namespace {
enum { F_OFFMASK = 1, F_W16 = 2, F_W16F = 4, F_GN = 8, F_PJ = 16 };
enum { IN_B, IN_HW, IN_CIN, IN_COUT, IN_COUT_PAD_MIN, IN_K, IN_STRIDE, IN_NSRC, IN_ACT, IN_FLAGS, IN_TILE64, IN_SPLITK, IN_DBG, IN_N };
enum { OUT_N = 8 };

ConvParams fill(const int* r) {
    const float* const dummy = reinterpret_cast<const float*>(0x1000);
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    const int k = r[IN_K], flags = r[IN_FLAGS];
    p.nsrc = r[IN_NSRC];
    p.Cin = r[IN_CIN];
    for (int s = 0; s < p.nsrc; ++s) {
        p.src[s] = dummy;
        p.src_c[s] = p.Cin / p.nsrc;
    }
    p.B = r[IN_B];
    p.H = p.W = r[IN_HW];
    p.KH = p.KW = k;
    p.stride = r[IN_STRIDE];
    p.pad = k / 2;
    p.Ho = (p.H + 2 * p.pad - k) / p.stride + 1;
    p.Wo = (p.W + 2 * p.pad - k) / p.stride + 1;
    p.K = k * k * p.Cin;
    p.Kpad = (p.K + 15) / 16 * 16;
    p.wp = dummy;
    p.Cout = r[IN_COUT];
    const int bn = cp_conv_tile_n(p.Cout);
    p.CoutPad = (p.Cout + bn - 1) / bn * bn;
    if (p.CoutPad < r[IN_COUT_PAD_MIN]) p.CoutPad = r[IN_COUT_PAD_MIN];
    p.scale = p.shift = dummy;
    p.act = r[IN_ACT];
    p.store = CP_STORE_NHWC;
    p.ldo = p.act == CP_ACT_SIGMOID_FROM ? p.CoutPad : p.Cout;  // (offset / mask maps keep their padded width)
    if (flags & F_W16) {
        p.w16_hi = p.w16_lo = dummy;
        p.Kpad16 = p.K;
    }
    if (flags & F_W16F) p.w16f_hi = p.w16f_lo = dummy;
    if (flags & F_OFFMASK) p.offmask = dummy;
    if (flags & F_GN) p.gn_in_a = p.gn_in_d = dummy;
    if (flags & F_PJ) {
        p.pj_src = dummy;
        p.pj_c = p.Cin;
        p.pj_w_hi = p.pj_w_lo = dummy;
    }
    if (r[IN_TILE64]) p.tile_m = p.tile_n = 64;
    p.splitk = r[IN_SPLITK];
    p.dbg = r[IN_DBG];
    return p;
}
}  // namespace

extern "C" {

int conv_select_row_ints(int* in, int* out) {
    *in = IN_N;
    *out = OUT_N;
    return 0;
}

// rows: n x IN_N ints -> out: n x OUT_N ints = cp_conv_variant, cp_conv16_supported, cp_conv16_variant, cp_conv16_project_supported,
// cp_conv_geometry's (tiles, K steps) for the float32 and for the f16x3 launch.  The two f16x3 answers that are only defined for a
// launch cp_conv16_supported accepts are -1 elsewhere.
void conv_select_eval(const int* rows, int n, int* out) {
    for (int i = 0; i < n; ++i) {
        const ConvParams p = fill(rows + (size_t)i * IN_N);
        int* o = out + (size_t)i * OUT_N;
        const bool ok16 = cp_conv16_supported(p);
        o[0] = cp_conv_variant(p);
        o[1] = ok16 ? 1 : 0;
        o[2] = ok16 ? cp_conv16_variant(p) : -1;
        o[3] = cp_conv16_project_supported(p) ? 1 : 0;
        cp_conv_geometry(p, false, &o[4], &o[5]);
        o[6] = o[7] = -1;
        if (ok16) cp_conv_geometry(p, true, &o[6], &o[7]);
    }
}

}  // extern "C"
