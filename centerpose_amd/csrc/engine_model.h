// What the engine's translation units share: the model's data types and work-space arena, the one place a ConvParams /
// DeconvLaunch is built, and the profiling bracket around a launch.
//   engine_pack.hip     parameter folding and packing (cp_model_create .. cp_model_finalize, cp_model_destroy)
//   engine_forward.hip  the forward pass and its kernel dispatch (forward_impl)
//   ops.hip             the stand-alone operators (cp_conv2d_nhwc, cp_conv_transpose2d_nhwc, cp_dcnv2_forward / _backward, cp_pose_heads_*)
//   engine.hip          the model's run-time C ABI and the one-line wrappers of the other modules
//   heads_bwd.hip, conv_bwd.hip  take conv_w_f32 / conv_params for the igemm.hip launches of their backward passes
// Everything here has C++ linkage (only the C ABI of include/centerpose_hip.h is exported unmangled).
#pragma once
#include "../../include/centerpose_hip.h"
#include "../../include/centerpose_hip_testing.h"
#undef CP_OK
#undef CP_ERR_INVALID
#undef CP_ERR_LAUNCH
#undef CP_ERR_ALLOC
#undef CP_ERR_STATE
#undef CP_DET_STRIDE
#undef CP_PNP_STRIDE
#undef CP_TRACK_STRIDE
#include "cp_common.h"
#include "engine_arena.h"  // align_up, Arena, Block

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace cp_engine {

// sets the calling thread's cp_last_error() text and returns `code` (one definition, engine.hip)
int fail(int code, const std::string& msg);

extern int g_default_precision;
extern int g_dbg;  // cp_set_debug: CP_SEL_* kernel-selection switches (include/centerpose_hip_testing.h)

// NHWC activation handle; memory returns to the arena when the last handle dies (the single stream
// orders reuse after the last enqueued consumer).
struct Tensor {
    std::shared_ptr<Block> blk;
    int C = 0, H = 0, W = 0;
    unsigned* amax = nullptr;  // 4-byte slot holding the float bits of max|x| (f16x3 mode; ConvParams::in_amax)
    float* ptr() const { return blk->a->base ? (float*)(blk->a->base + blk->off) : nullptr; }
    bool valid() const { return (bool)blk; }
};

struct ConvW {
    float* wp = nullptr;           // [Kpad][CoutPad]
    const float* scale = nullptr;  // [CoutPad] or nullptr
    const float* shift = nullptr;  // [CoutPad] or nullptr
    int Cin = 0, CinP = 0, Cout = 0, CoutPad = 0, KH = 0, KW = 0, K = 0, Kpad = 0;
    void* w16_hi = nullptr;  // split-f16 copies [CoutPad][K] (only when every K-step of 32 stays inside one tap)
    void* w16_lo = nullptr;
    int Kpad16 = 0;
    void* w16f_hi = nullptr;  // DCN main convolutions: the same in MFMA fragment order (dcn16p.hip)
    void* w16f_lo = nullptr;
    // per-output-channel power-of-two pre-scale of the split-f16 copies: rows are stored times wfwd[co] = 2^e,
    // winv = 2^-e, scale16 = (scale or 1) * winv is what the f16x3 kernels' epilogue multiplies with
    float* wfwd = nullptr;
    float* winv = nullptr;
    float* scale16 = nullptr;
};

struct LowcW {
    void* hi = nullptr;
    void* lo = nullptr;
    float* scale16 = nullptr;  // folded BatchNorm scale x 2^-e of the fragment rows
};

struct DeformW {
    ConvW offset;  // conv_offset_mask (27 -> 32 padded), shift = bias
    ConvW main;    // DCN weight, scale/shift = folded bias + BN
};

// dense ConvTranspose2d(k=4, s=2, p=1) + folded BatchNorm of a resdcn deconv stage (deconv16.hip)
struct DeconvW {
    float* wf = nullptr;           // float32 sub-kernels [4][CoutPad][4*Cin]
    void* hi = nullptr;            // split-f16 copies, rows times 2^e per output channel
    void* lo = nullptr;
    const float* scale = nullptr;  // [CoutPad] folded BatchNorm scale
    float* scale16 = nullptr;      // scale * 2^-e
    const float* shift = nullptr;
    int Cin = 0, Cout = 0;
};

struct HeadW {
    std::string name;
    int classes = 0;
    ConvW c0, c1;
    void* w2_hi = nullptr;  // fused-head form of c1 (cp_launch_pack_head_w2); null when the pair is not eligible
    void* w2_lo = nullptr;
    float* w2_inv = nullptr;  // [32] 2^-e per final channel (+ [32] 2^e used while packing)
    float* gn_gamma = nullptr;
    float* gn_beta = nullptr;
};

// resdcn depth -> (Bottleneck?, blocks per layer): resnet_spec of resnet_dcn.py
inline bool resnet_spec(int depth, bool* bottleneck, int* blocks) {
    static const int spec[5][5] = {{18, 2, 2, 2, 2}, {34, 3, 4, 6, 3}, {50, 3, 4, 6, 3}, {101, 3, 4, 23, 3}, {152, 3, 8, 36, 3}};
    for (const auto& r : spec)
        if (r[0] == depth) {
            *bottleneck = depth >= 50;
            for (int i = 0; i < 4; ++i) blocks[i] = r[i + 1];
            return true;
        }
    return false;
}

}  // namespace cp_engine

struct cp_model {
    std::string arch;
    bool gru = false, tracking = false, finalized = false, hourglass = false;
    int resnet = 0;  // resdcn_N: N (resnet_dcn.py), else 0
    int precision = cp_engine::g_default_precision;
    int head_conv = 256;
    std::vector<std::pair<std::string, int>> heads;
    std::map<std::string, std::vector<float>> params;  // host copies until finalize
    std::map<std::string, cp_engine::ConvW> convs;
    std::map<std::string, cp_engine::DeformW> deforms;
    std::map<std::string, float*> ups;    // IDAUp's depth-wise up-sampling kernels [C][k][k] as in the checkpoint
    std::map<std::string, float*> ups_t;  // ... and as [tap][C]
    std::map<std::string, cp_engine::DeconvW> deconvs;
    std::vector<cp_engine::HeadW> headw;
    // every fused head of the model in ONE launch (they all read the same feature map): the heads' 3x3 fragments,
    // scale / shift, 1x1 fragments and w2_inv tables concatenated along N (ConvParams::fuse_ngroups)
    struct HeadGroup {
        bool ok = false;
        void* w16f_hi = nullptr;
        void* w16f_lo = nullptr;
        void* w2_hi = nullptr;
        void* w2_lo = nullptr;
        float* scale16 = nullptr;
        float* shift = nullptr;
        float* w2_inv = nullptr;
        int Cin = 0, hid = 0, Kpad16 = 0;
        void* w16_hi = nullptr;  // the 3x3 weights as [co][k] rows as well (pixel-list kernel), reg_group only
        void* w16_lo = nullptr;
        std::vector<int> idx;    // the group's heads (indices into headw) in concatenation order
    } head_group;
    // cp_model_detect_lean: hm + hm_hp (dense), and every other head (first lean_ncentre: read at the centre peaks; then hp_offset)
    HeadGroup hm_group, reg_group;
    int lean_ncentre = 0;
    // one lean detect call: what forward_impl's head stage does instead of the dense launch of every head (engine_forward.hip)
    struct LeanCall {
        float* const* table_out;  // per head of the model: its compact table, or nullptr (hm, hm_hp, heads not wanted)
        float* pk_score;          // [B][J+1][K]
        int* pk_ind;
        void* scratch;            // tiled peaks' candidates, then the pixel-list launches' slabs
        float* dense_slabs;       // where cp_model_dense_heads may keep its slabs (models whose grouped launch needs them), or nullptr
        int K, rep_mode, fit_gaussian, legacy_bool_mask;
        float balance;
        float* det;
    };
    const LeanCall* lean = nullptr;
    bool lean_taken = false;  // set by the head stage when it ran (or, dry, would run) the lean sequence
    int lean_key[5] = {0, 0, 0, -1, -1};  // (B, H, W, g_dbg, precision) of the cached cp_model_lean_supported answer
    bool lean_ok = false;
    // the feature map the heads of the last lean detect read: it stays in the caller's workspace until the next call that uses it
    struct KeptFeat {
        const float* ptr = nullptr;
        unsigned* amax = nullptr;
        int B = 0, H = 0, W = 0, C = 0;  // (H, W: of the feature map)
        float* slabs = nullptr;          // LeanCall::dense_slabs of that call
    } kept;
    std::map<std::vector<uint64_t>, KeptFeat> graph_kept;  // ... per captured lean graph (a replay does not run the host code)
    std::map<std::string, cp_engine::LowcW> lowc;  // hi / lo weight fragments of the lowc.hip layers
    int ws_key[4] = {0, 0, 0, -1};  // (B, H, W, g_dbg) of the cached work-space query below
    size_t ws_cached = 0;
    // One form of the launch sequence for the work-space query (switches, previous-frame inputs and taps may select any of them
    // later: cp_model_workspace_bytes).  A real pass, and cp_model_lean_supported's dry one, leaves every field at its default.
    struct DryForm {
        bool stem_level0_fused = false;  // the fused stem + level0 launch where the model allows it (a real pass: no previous-frame input)
        bool tap_routing = false;        // what any tap causes whatever it names: the fused heads are off
        enum { IDA_ALL, IDA_NONE, IDA_BOUNDARY } idaup = IDA_ALL;  // IDAUp's up-sample + add inside the preceding node at every site that
                                         // can / at none (a tap on a node) / only between dla_up and ida_up (a tap on another node than that one)
        bool project_unfused = false;    // the level entries' projection as a launch of its own (a tap on one selects that)
        bool no_pooled_producer = false; // every stride-2 entry with its maxpool2 launch (no producer writes the pooled copy)
    } form;
    float stem_bound_l = 0.f, stem_bound_s = 0.f;  // |base_layer out| <= stem_bound_l * max|image| + stem_bound_s (fused stem + level0)
    cp_engine::ConvW gru_x, gru_h;
    void* gru_h16_hi = nullptr;  // hidden-side GRU weights re-ordered [tile][r|z|n][32] for the fused-gate kernel
    void* gru_h16_lo = nullptr;
    void* gru_h16f_hi = nullptr;  // ... and in MFMA fragment order (halo16.hip)
    void* gru_h16f_lo = nullptr;
    float* gru_h16_fwd = nullptr;  // [192] per-row 2^e of the fused-order copies, and the matching 2^-e
    float* gru_h16_inv = nullptr;
    std::vector<void*> device_allocs;
    cp_engine::Arena arena;
    // forward-call state
    hipStream_t stream = nullptr;
    int B = 0;
    bool dry = false;
    int status = CP_OK;
    int maxpool2_launches = 0;  // stand-alone 2x2 max-pool launches of the last pass, dry or real (cp_model_maxpool_launches)
    const char* tap_name = nullptr;
    float* tap_out = nullptr;
    int* tap_dims = nullptr;
    float* feat_out = nullptr;  // cp_model_features: the heads' input goes here (NHWC) and the pass ends before the heads
    // optional per-launch profiling of the implicit-GEMM kernels (HIP events on the launch stream)
    struct ProfRec {
        int variant;
        int role = 0;  // CP_ROLE_*
        double flops, bytes;
        int M, N, K, kh, stride;
        hipEvent_t e0, e1;
    };
    std::map<std::vector<uint64_t>, hipGraphExec_t> graphs;  // captured detect() launches, keyed by every argument
    bool profile = false;
    std::vector<ProfRec> prof;
    double roles[CP_NUM_ROLES * 4] = {0};  // per-role totals of the last cp_model_profile_read
    std::vector<hipEvent_t> event_pool;
    hipEvent_t get_event() {
        if (!event_pool.empty()) {
            hipEvent_t e = event_pool.back();
            event_pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};

namespace cp_engine {

int forward_impl(cp_model* m, hipStream_t stream, int B, int H, int W, const float* images, const float* pre_img,
                 const float* pre_hm, const float* pre_hm_hp, float* const* head_out, int sigmoid_hm, void* ws,
                 size_t ws_bytes, bool dry);

int kept_dense_heads(cp_model* m, hipStream_t stream, float* const* head_out);
int kept_heads_at(cp_model* m, hipStream_t stream, const int* index, int n, float* const* table_out, float* slabs);

// slab bytes of a pixel-list launch of every head of cp_model::reg_group over `rows` rows (two hidden slices per head)
inline size_t lean_slab_bytes(const cp_model* m, size_t rows) {
    size_t planes = 0;
    for (int i : m->reg_group.idx) planes += (size_t)(m->reg_group.hid / 128) * m->headw[i].classes;
    return align_up(planes * rows * sizeof(float), 256);
}

// does the grouped head launch write finished maps (halo16: fuse_final), or slabs + a reduction launch?
inline bool lean_finished_maps(const cp_model* m) {
    return m->head_group.Cin == 64 && m->head_group.hid == 256 && !(g_dbg & CP_SEL_HEADS_SLABS);
}

// The one profiling bracket: runs `launch` (-> CP_* code).  While the model is profiling, `describe` fills in what the launch
// is charged for (variant, role, flops, bytes, shape) and two events on `s` around it time it for cp_model_profile_read.
// Both are inlined lambdas: nothing is evaluated, allocated or copied for the record when profiling is off.
template <class D, class F>
inline int timed(cp_model* m, hipStream_t s, D&& describe, F&& launch) {
    if (!m->profile) return launch();
    cp_model::ProfRec r;
    describe(r);
    r.e0 = m->get_event();
    r.e1 = m->get_event();
    (void)hipEventRecord(r.e0, s);
    const int rc = launch();
    (void)hipEventRecord(r.e1, s);
    m->prof.push_back(r);
    return rc;
}

// ConvW of a float32 weight as cp_launch_pack_weight lays it out in a caller's buffer: wp [Kpad][CoutPad], K = KH KW Cin rounded
// up to the kernels' K step and Cout to the launch's N tile; no f16x3 operands (cp_pack_f16x3 of ops.hip adds them)
inline ConvW conv_w_f32(float* wp, const float* scale, const float* shift, int Cin, int Cout, int KH, int KW) {
    ConvW w;
    w.wp = wp;
    w.scale = scale;
    w.shift = shift;
    w.Cin = w.CinP = Cin;
    w.Cout = Cout;
    w.CoutPad = (int)align_up((size_t)Cout, cp_conv_tile_n(Cout));
    w.KH = KH;
    w.KW = KW;
    w.K = KH * KW * Cin;
    w.Kpad = (int)align_up((size_t)w.K, 16);
    return w;
}

// The one place a ConvParams is built.  Zeroed, then what every convolution launch has in common: the sources (a virtual
// concat along C, all B x H x W), the geometry, and the float32 form of the weights with their epilogue.  The caller adds
// only what is its own (residual, offsets, fusion pointers, GroupNorm hooks, split-K, where the output goes).
inline ConvParams conv_params(int B, int H, int W, const float* const* src, const int* src_c, int nsrc, const ConvW& w,
                              int stride, int pad, int act) {
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.nsrc = nsrc;
    for (int i = 0; i < nsrc; ++i) {
        p.src[i] = src[i];
        p.src_c[i] = src_c[i];
        p.Cin += src_c[i];
    }
    p.B = B;
    p.H = H;
    p.W = W;
    p.Ho = (H + 2 * pad - w.KH) / stride + 1;
    p.Wo = (W + 2 * pad - w.KW) / stride + 1;
    p.KH = w.KH;
    p.KW = w.KW;
    p.stride = stride;
    p.pad = pad;
    p.K = w.K;
    p.Kpad = w.Kpad;
    p.wp = w.wp;
    p.Cout = w.Cout;
    p.CoutPad = w.CoutPad;
    p.scale = w.scale;
    p.shift = w.shift;
    p.act = act;
    p.dbg = g_dbg;
    return p;
}
// Second step, after the caller's own fields: attaches w's split-f16 operands, and where the f16x3 kernels take the launch --
// `f16x3` (the caller's precision) and cp_conv16_supported(p) as p stands now, or an `f16_only` kernel that has no float32
// form (fused heads, fused GRU step) -- switches the epilogue to scale16 and hands over the sources' |max| slots.
// Returns whether they take it.
inline bool conv_params_f16(ConvParams& p, const ConvW& w, const unsigned* const* in_amax, bool f16x3, bool f16_only = false) {
    p.w16_hi = w.w16_hi;
    p.w16_lo = w.w16_lo;
    p.w16f_hi = w.w16f_hi;
    p.w16f_lo = w.w16f_lo;
    p.Kpad16 = w.Kpad16;
    if (!f16_only && !(f16x3 && cp_conv16_supported(p))) return false;
    p.scale = w.scale16;
    for (int i = 0; i < p.nsrc; ++i) p.in_amax[i] = in_amax[i];
    return true;
}

// ... and a DeconvLaunch: x [B,H,W,d.Cin] -> out [B,2H,2W,d.Cout], operands and scale of the chosen arithmetic
inline DeconvLaunch deconv_launch(const DeconvW& d, bool f16x3, const float* x, const unsigned* in_amax, int B, int H, int W,
                                  float* out, unsigned* out_amax, bool relu) {
    DeconvLaunch l;
    std::memset(&l, 0, sizeof(l));
    l.f16x3 = f16x3;
    l.x = x;
    l.wf = d.wf;
    l.w_hi = d.hi;
    l.w_lo = d.lo;
    l.scale = f16x3 ? d.scale16 : d.scale;
    l.shift = d.shift;
    l.out = out;
    l.in_amax = in_amax;
    l.out_amax = out_amax;
    l.B = B;
    l.H = H;
    l.W = W;
    l.Cin = d.Cin;
    l.Cout = d.Cout;
    l.relu = relu;
    return l;
}

}  // namespace cp_engine
