// The forward pass: a fixed sequence of HIP kernel launches on the caller's stream out of a caller-provided workspace
// (deterministic arena, no allocation, no sync).  Fwd decides per layer which kernel runs; a dry run of the same code is the
// work-space query.  A generic conv is asked for with a ConvCall; plan() alone turns one into ConvParams + kernel + accepted
// fusions, for conv() and for the predicates that ask about a launch ahead of time (upadd_fusable, project_fusable) alike.
//
// Topology follows the reference modules (paths relative to the reference's src/lib/models/networks):
//   DLA.forward pose_dla_dcn.py:310-322, Tree.forward :211-224, Root :160-168, BasicBlock :48-62,
//   DLAUp :437-443, IDAUp :411-417, DeformConv :386-389 (DCN: DCNv2/dcn_v2.py:118-128),
//   DLASeg.forward :523-570, ConvGRU convGRU.py:72-94, GroupNorm GN.py:4-9.
#include "engine_model.h"

using namespace cp_engine;

namespace {

// split-K policy: launches with fewer output tiles than kSplitTiles (and >= 8 K steps) are cut into K slices until
// about kSplitTarget workgroups exist
constexpr int kSplitTiles = 128, kSplitTarget = 384;  // (384 / 512 measured: B=32 equal, hourglass B=1 latency +7 %)
// lean detect (heads at the peaks only) from this many output pixels per call: it trades five sevenths of the dense head launch,
// which shrinks with the batch, for dependent small launches between peaks and association, which do not.  Measured on dla_34 at
// 512 x 512 (graph replay, p50, lean - dense): B = 1 (16384 pixels) +0.011 ms, B = 2 -0.049, B = 4 -0.146, B = 8 -0.333, B = 16 -0.716
// (profiles/lean_detect_ab.txt).
constexpr long kLeanMinPixels = 32768;
// stands for the address of a tensor that is not there (yet): planning and eligibility checks look at null / non-null only
float* const kDryPtr = (float*)0x1000;

// ------------------------------------ forward -------------------------------------------------
struct Fwd {
    cp_model* m;
    int B;
    hipStream_t s;
    // |max| slots of this forward's tensors (f16x3 range-safe scaling, ConvParams::in_amax): one zeroed block at the
    // start of the arena, a slot per Tensor in creation order
    static constexpr int kMaxSlots = CP_AMAX_STRIDE;
    static constexpr size_t kSlotBytes = (size_t)CP_AMAX_SUB * CP_AMAX_STRIDE * sizeof(unsigned);
    Tensor slots_t;
    unsigned* slots = nullptr;
    int nslots = 0;
    void init_slots() {
        slots_t.blk = std::make_shared<Block>(&m->arena, kSlotBytes);
        if (m->dry || m->precision != CP_PREC_F16X3 || (g_dbg & CP_SEL_NO_PRESCALE)) return;  // operands used unscaled (range-safety tests)
        slots = (unsigned*)slots_t.ptr();
        if (hipMemsetAsync(slots, 0, kSlotBytes, s) != hipSuccess) chk(CP_ERR_LAUNCH);
    }
    unsigned* new_slot() {
        if (!slots) return nullptr;
        if (nslots >= kMaxSlots) {
            chk(fail(CP_ERR_STATE, "out of |max| slots"));
            return nullptr;
        }
        return slots + nslots++;
    }
    // |max| of a caller-owned input (network images): one extra read of the tensor
    unsigned* input_slot(const float* x, size_t n) {
        unsigned* sl = new_slot();
        if (sl) chk(cp_launch_absmax(x, n, sl, s));
        return sl;
    }

    void chk(int rc) {
        if (rc != CP_OK && m->status == CP_OK) m->status = rc;
    }
    // every profiled launch goes through here: `describe` (what the launch is charged for) only runs while profiling
    template <class D, class F>
    void timed(D&& describe, F&& launch) {
        chk(cp_engine::timed(m, s, describe, launch));
    }
    Tensor make(int C, int H, int W) {
        Tensor t;
        t.C = C;
        t.H = H;
        t.W = W;
        t.blk = std::make_shared<Block>(&m->arena, (size_t)B * H * W * C * sizeof(float));
        t.amax = new_slot();
        return t;
    }
    void tap(const char* name, const Tensor& t, int c_valid = 0) {
        if (m->dry || !m->tap_name || std::strcmp(name, m->tap_name) != 0) return;
        const int C = c_valid ? c_valid : t.C;
        chk(cp_launch_nhwc_to_nchw(t.ptr(), m->tap_out, B, C, t.H, t.W, t.C, s));
        if (m->tap_dims) {
            m->tap_dims[0] = C;
            m->tap_dims[1] = t.H;
            m->tap_dims[2] = t.W;
        }
    }
    void tap(const std::string& name, const Tensor& t, int c_valid = 0) { tap(name.c_str(), t, c_valid); }
    bool tapped() const { return m->tap_name || m->form.tap_routing; }  // any tap (or the query's form of one): the fused heads are off
    // cp_model_features: hands the heads' input to the caller; true = the pass ends here, no head is launched
    bool features_only(const Tensor& t) {
        if (!m->feat_out || m->dry) return false;
        if (hipMemcpyAsync(m->feat_out, t.ptr(), (size_t)B * t.H * t.W * t.C * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
            chk(CP_ERR_LAUNCH);
        return true;
    }

    // conv3x3 (+bias, ReLU) -> conv1x1 (+bias, optional sigmoid) of a prediction head in one kernel + a slice reduction;
    // returns false (nothing launched) when the launch would want split-K or the shapes are not eligible
    bool fused_head(const HeadW& hw, const Tensor& x, bool sigmoid, float* out_nchw) {
        const ConvW& w = hw.c0;
        if (x.C != w.CinP) return false;
        const float* src = x.ptr();
        ConvParams p = conv_params(B, x.H, x.W, &src, &x.C, 1, w, 1, 1, CP_ACT_RELU);
        p.splitk = 1;
        p.fuse_w2_hi = hw.w2_hi;
        p.fuse_w2_lo = hw.w2_lo;
        p.fuse_w2_inv = hw.w2_inv;
        p.fuse_c2 = hw.classes;
        conv_params_f16(p, w, &x.amax, true, true);
        if (w.KH != 3 || w.KW != 3 || !cp_head_fuse_supported(p, hw.classes)) return false;
        int tiles = 0, nk = 0;
        cp_conv_geometry(p, true, &tiles, &nk);
        if (tiles < kSplitTiles && nk >= 8) return false;  // small launches keep the split-K path (conv())
        const int slices = p.CoutPad / 128;
        Tensor slabs = make(slices * hw.classes, p.Ho, p.Wo);
        p.fuse_out = slabs.ptr();
        auto launch = [&]() -> int {
            int rc = cp_launch_conv16_fused_head(p, s);
            if (rc == CP_OK)
                rc = cp_launch_head_reduce(slabs.ptr(), hw.c1.shift, out_nchw, slices, hw.classes, B, p.Ho * p.Wo,
                                           sigmoid ? 1 : 0, s);
            return rc;
        };
        if (m->dry) return true;
        timed([&](cp_model::ProfRec& r) {
            r.variant = cp_conv16_fused_head_variant(p);
            r.role = CP_ROLE_HEAD;
            const double M = (double)B * p.Ho * p.Wo;
            r.flops = 2.0 * M * w.Cout * (double)(w.KH * w.KW * w.Cin) + 2.0 * M * hw.classes * (double)w.Cout;
            // algorithmic bytes: input once + final maps once + both weight sets (the hidden tensor is not counted:
            // it is not part of the head's definition, only of the unfused implementation)
            r.bytes = 4.0 * ((double)B * x.H * x.W * w.Cin + M * hw.classes + (double)w.KH * w.KW * w.Cin * w.Cout +
                             (double)w.Cout * hw.classes);
            r.M = (int)M; r.N = w.Cout; r.K = w.KH * w.KW * w.Cin; r.kh = w.KH; r.stride = 1;
        }, launch);
        return true;
    }

    // every fused head of the model in one launch + one slice reduction (cp_model::head_group); false = nothing launched.
    // A lean detect call (cp_model::lean) runs its own head stage here instead.
    bool fused_heads_grouped(const Tensor& x, float* const* head_out, int sigmoid_hm) {
        if (m->lean) return lean_heads(x, head_out);
        return grouped_launch(m->head_group, x.ptr(), x.amax, x.C, x.H, x.W, head_out, sigmoid_hm, nullptr);
    }

    // Per-head tables of a launch over the heads g.idx[first, first + n), side by side along N: each head's final width and first slab
    // plane for the kernel (fuse_gc2 / fuse_gbase) and the slice reduction (rg, with the bias), and what the launch is charged for over
    // M rows, added head by head to flops / bytes.  Returns the slab planes.
    int head_tables(const cp_model::HeadGroup& g, int first, int n, double M, ConvParams& p, HeadReduceGroup& rg, double& flops, double& bytes) {
        std::memset(&rg, 0, sizeof(rg));
        rg.n = n;
        rg.slices = p.fuse_gtiles;
        int planes = 0;
        for (int i = 0; i < n; ++i) {
            const HeadW& hw = m->headw[g.idx[first + i]];
            p.fuse_gc2[i] = rg.c2[i] = hw.classes;
            p.fuse_gbase[i] = rg.base[i] = planes;
            planes += p.fuse_gtiles * hw.classes;
            rg.bias[i] = hw.c1.shift;
            flops += 2.0 * M * g.hid * (9.0 * g.Cin) + 2.0 * M * hw.classes * (double)g.hid;
            bytes += 4.0 * (M * hw.classes + 9.0 * g.Cin * g.hid + (double)g.hid * hw.classes);
        }
        return planes;
    }

    // the heads of group g (a subset of the model's heads, cp_model::HeadGroup::idx) on the feature map `src` in one halo16
    // launch; head_out is indexed like the model's heads.  The choice of the kernel form looks at the model's whole head set, not
    // at g: a head's map must not depend on which other heads share its launch.  slab_mem: where the slabs + reduction form keeps
    // its slabs (nullptr: in the arena).
    bool grouped_launch(const cp_model::HeadGroup& g, const float* src, unsigned* src_amax, int C, int H, int W,
                        float* const* head_out, int sigmoid_hm, float* slab_mem) {
        const int n = (int)g.idx.size(), n_all = (int)m->headw.size();
        if (!g.ok || m->precision != CP_PREC_F16X3 || tapped() || (g_dbg & (CP_SEL_NO_HEAD_FUSION | CP_SEL_HEADS_PER_HEAD_LAUNCH)) || C != g.Cin)
            return false;
        ConvW w;  // the heads' 3x3 layers side by side along N: fragment-ordered f16x3 operands only
        w.KH = w.KW = 3;
        w.K = w.Kpad = w.Kpad16 = g.Kpad16;
        w.Cout = w.CoutPad = n * g.hid;
        w.scale16 = g.scale16;
        w.shift = g.shift;
        w.w16f_hi = g.w16f_hi;
        w.w16f_lo = g.w16f_lo;
        ConvParams p = conv_params(B, H, W, &src, &C, 1, w, 1, 1, CP_ACT_RELU);
        const unsigned* amax_c = src_amax;
        conv_params_f16(p, w, &amax_c, true, true);
        p.splitk = 1;
        p.fuse_w2_hi = g.w2_hi;
        p.fuse_w2_lo = g.w2_lo;
        p.fuse_w2_inv = g.w2_inv;
        p.fuse_ngroups = n;
        p.fuse_gtiles = g.hid / 128;
        p.fuse_out = kDryPtr;  // (for the eligibility check)
        // the kernel walks a head's hidden tiles and writes the finished maps itself (CP_SEL_HEADS_SLABS: slabs + reduction
        // launch); 2: every head of a patch in one workgroup (one staging for all of them) -- when the patches alone fill the
        // device several times over; below that (small batches, CP_SEL_HEADS_WG_PER_HEAD) one workgroup per patch and head
        p.fuse_final = (g.Cin == 64 && g.hid == 256 && !(g_dbg & CP_SEL_HEADS_SLABS))
                           ? (((g_dbg & CP_SEL_HEADS_WG_PER_HEAD) || B * (H / 8) * (W / 16) < 2048) ? 1 : 2) : 0;
        if (!cp_halo16_fused_head_supported(p)) return false;
        if (B * (H / 8) * (W / 16) * (n_all * g.hid / 128) < kSplitTiles) return false;  // small maps: per-head split-K path
        HeadReduceGroup rg;
        double flops = 0.0, bytes = 0.0;
        const double M = (double)B * H * W;
        const int planes = head_tables(g, 0, n, M, p, rg, flops, bytes);
        bytes += 4.0 * M * g.Cin;  // the shared input is read once
        for (int i = 0; i < n; ++i) {
            const HeadW& hw = m->headw[g.idx[i]];
            p.fuse_gsig[i] = rg.sigmoid[i] = sigmoid_hm && (hw.name == "hm" || hw.name == "hm_hp");
            p.fuse_gbias[i] = rg.bias[i];
            p.fuse_gout[i] = rg.out[i] = m->dry ? nullptr : head_out[g.idx[i]];
        }
        Tensor slabs;
        if (!p.fuse_final && !slab_mem) slabs = make(planes, H, W);
        if (m->dry) return true;
        p.fuse_out = p.fuse_final ? nullptr : slab_mem ? slab_mem : slabs.ptr();
        auto launch = [&]() -> int {
            int rc = cp_launch_halo16_fused_head(p, s);
            if (rc == CP_OK && !p.fuse_final) rc = cp_launch_head_reduce_grouped(p.fuse_out, rg, B, H * W, s);
            return rc;
        };
        timed([&](cp_model::ProfRec& r) {
            r.variant = CP_VARIANT_HALO_HEAD;
            r.role = CP_ROLE_HEAD;
            r.flops = flops;
            r.bytes = bytes;
            r.M = (int)M; r.N = p.CoutPad; r.K = 9 * g.Cin; r.kh = 3; r.stride = 1;
        }, launch);
        return true;
    }

    // Heads [first, first + count) of cp_model::reg_group evaluated at a list of pixels of the feature map `src` only (per image:
    // `rpi` entries at index + b * stride) in one launch of the pixel-list kernel + one slice reduction:
    // table_out[model head] receives [Bout][classes][Kt] with Bout * Kt = B * rpi rows in list order.  slabs: lean_slab_bytes().
    void heads_at_rows(int first, int count, const float* src, unsigned* src_amax, int C, int H, int W, const int* index,
                       int stride, int rpi, int Bout, int Kt, float* const* table_out, float* slabs) {
        const auto& g = m->reg_group;
        const size_t wbytes = (size_t)g.hid * g.Kpad16 * 2, w2bytes = (size_t)g.hid * 32 * 2;
        ConvW w;  // the heads' 3x3 layers side by side along N, [co][k] rows
        w.KH = w.KW = 3;
        w.K = w.Kpad = w.Kpad16 = g.Kpad16;
        w.Cin = w.CinP = g.Cin;
        w.Cout = w.CoutPad = count * g.hid;
        w.scale16 = g.scale16 + (size_t)first * g.hid;
        w.shift = g.shift + (size_t)first * g.hid;
        w.w16_hi = (char*)g.w16_hi + first * wbytes;
        w.w16_lo = (char*)g.w16_lo + first * wbytes;
        ConvParams p = conv_params(B, H, W, &src, &C, 1, w, 1, 1, CP_ACT_RELU);
        const unsigned* amax_c = src_amax;
        conv_params_f16(p, w, &amax_c, true, true);  // the dense launch's pre-scale: the same operands in the first product
        p.splitk = 1;
        p.fuse_w2_hi = (char*)g.w2_hi + first * w2bytes;
        p.fuse_w2_lo = (char*)g.w2_lo + first * w2bytes;
        p.fuse_w2_inv = g.w2_inv + (size_t)first * 64;
        p.fuse_ngroups = count;
        p.fuse_gtiles = g.hid / 128;
        p.fuse_out = slabs;
        p.row_index = index;
        p.rows_per_image = rpi;
        p.row_index_stride = stride;
        HeadReduceGroup rg;
        const double M = (double)B * rpi;
        double flops = 0.0, bytes = 4.0 * M * 9.0 * g.Cin;
        head_tables(g, first, count, M, p, rg, flops, bytes);
        for (int i = 0; i < count; ++i) {
            rg.out[i] = table_out[g.idx[first + i]];
            if (!rg.out[i]) {
                chk(fail(CP_ERR_INVALID, "heads at pixels: no table for head " + m->headw[g.idx[first + i]].name));
                return;
            }
        }
        timed([&](cp_model::ProfRec& r) {
            r.variant = CP_VARIANT_HEAD_ROWS;
            r.role = CP_ROLE_HEAD;
            r.flops = flops;  // what the launch executes: its rows only
            r.bytes = bytes;
            r.M = (int)M; r.N = p.CoutPad; r.K = 9 * g.Cin; r.kh = 3; r.stride = 1;
        }, [&]() -> int {
            int rc = cp_launch_conv16_fused_head_rows(p, s);
            if (rc == CP_OK) rc = cp_launch_head_reduce_grouped(slabs, rg, Bout, Kt, s);
            return rc;
        });
    }

    // The head stage of cp_model_detect_lean: hm + hm_hp densely -> peaks -> the other heads at the peaks' pixels only (what the
    // decode reads of them, decode.hip: assoc_kernel) -> records.  The feature map stays where it is for cp_model_dense_heads.
    bool lean_heads(const Tensor& x, float* const* head_out) {
        const cp_model::LeanCall& lc = *m->lean;
        const auto& gr = m->reg_group;
        const int J = 8, K = lc.K, nc = m->lean_ncentre, nr = (int)gr.idx.size();
        if (!gr.ok || !m->hm_group.ok || (long)B * x.H * x.W < kLeanMinPixels || !grouped_launch(m->hm_group, x.ptr(), x.amax, x.C, x.H, x.W, head_out, 1, nullptr)) {
            chk(fail(CP_ERR_STATE, "lean detect: this model / shape / switch setting runs the dense heads (cp_model_lean_supported)"));
            return true;
        }
        m->lean_taken = true;
        if (m->dry) return true;
        m->kept.ptr = x.ptr();
        m->kept.amax = x.amax;
        m->kept.B = B; m->kept.H = x.H; m->kept.W = x.W; m->kept.C = x.C;
        m->kept.slabs = lc.dense_slabs;
        float *hm = nullptr, *hm_hp = nullptr;
        const float* tb[11] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        static const char* names[11] = {"hm", "hps", "wh", "hps_uncertainty", "scale", "scale_uncertainty", "reg", "hm_hp",
                                        "hp_offset", "tracking", "tracking_hp"};
        for (size_t i = 0; i < m->headw.size(); ++i) {
            if (m->headw[i].name == "hm") hm = head_out[i];
            if (m->headw[i].name == "hm_hp") hm_hp = head_out[i];
            for (int j = 0; j < 11; ++j)
                if (m->headw[i].name == names[j]) tb[j] = lc.table_out[i];
        }
        const size_t cand = cp_decode_cand_bytes(B, J, x.H, x.W, K);
        if (cand == (size_t)-1 || !tb[1] || !tb[2]) {
            chk(fail(CP_ERR_INVALID, "lean detect: unsupported decode shape, or no table for hps / wh"));
            return true;
        }
        float* slabs = (float*)((char*)lc.scratch + align_up(cand, 256));
        const double hw = (double)x.H * x.W;
        auto decode_rec = [&](cp_model::ProfRec& r, double bytes) {
            r.variant = CP_VARIANT_NONE;
            r.role = CP_ROLE_DECODE;
            r.flops = 0.0;
            r.bytes = bytes;
            r.M = B; r.N = K; r.K = (int)hw; r.kh = 0; r.stride = 0;
        };
        timed([&](cp_model::ProfRec& r) { decode_rec(r, (double)B * 9.0 * hw * 4); },
              [&]() { return cp_launch_decode_peaks(s, B, J, x.H, x.W, hm, hm_hp, K, 0, lc.pk_score, lc.pk_ind, lc.scratch); });
        // centre-indexed heads at the K peaks of map 0, hp_offset at the K peaks of each of the J joint maps
        heads_at_rows(0, nc, x.ptr(), x.amax, x.C, x.H, x.W, lc.pk_ind, (J + 1) * K, K, B, K, lc.table_out, slabs);
        if (nr > nc)
            heads_at_rows(nc, 1, x.ptr(), x.amax, x.C, x.H, x.W, lc.pk_ind + K, (J + 1) * K, J * K, B * J, K, lc.table_out, slabs);
        timed([&](cp_model::ProfRec& r) { decode_rec(r, (double)B * (K * 60.0 * 4 + 8.0 * K * 2 * 4 + (double)K * CP_DET_STRIDE * 4)); },
              [&]() {
                  return cp_launch_decode_assoc(s, B, J, x.H, x.W, tb[1], tb[2], tb[3], tb[4], tb[5], tb[6], hm_hp, tb[8], tb[9], tb[10],
                                                lc.pk_score, lc.pk_ind, K, lc.rep_mode, lc.fit_gaussian, lc.balance,
                                                lc.legacy_bool_mask, 1, lc.det);
              });
        return true;
    }

    // IDAUp's next up-sample + add, done by the epilogue of the node that produces `add` (ida()): the conv's output tensor is
    // u = act(conv) + up(t), the node's own output does not exist
    struct UpFuse { const Tensor* t; const float* wt; int f; };  // (wt: cp_model::ups_t, f: the factor)
    // A level entry's 1x1 projection (Tree.project) computed by the block's conv2, which would otherwise read it back as its
    // residual (halo16.hip, ConvParams::pj_src): the projected tensor and its launch do not exist
    struct ProjFuse { const Tensor* bottom; const ConvW* w; };  // (w: <p>.project)
    // GroupNorm of a dlav1 head around its two convs, at most one form per call
    struct GroupNormPart {
        double* stats_out = nullptr;                                    // the 3x3's epilogue accumulates the statistics
        const float *mr = nullptr, *gamma = nullptr, *beta = nullptr;   // the 1x1's loader normalises from mean / rstd per group (float32)
        const float *a = nullptr, *d = nullptr;                         // ... or pre-folded to relu(a x + d) per (image, channel) (f16x3),
        const unsigned* bound = nullptr;                                // with a bound on its |max| for the loader's pre-scale
    };
    // One request to conv(): everything it is told arrives here, nothing is kept from one call to the next.  Past `act` every
    // field defaults to "none" and a call site names the ones it uses.
    struct ConvCall {
        const ConvW& w;
        std::vector<const Tensor*> srcs;  // a virtual concat along C
        int stride, pad, act;
        const Tensor* res = nullptr;      // added before the activation
        const Tensor* offmask = nullptr;  // DCNv2: the offset / mask map of the same pixels
        int act_from = 0;                 // CP_ACT_SIGMOID_FROM: first channel of the sigmoid
        float* out_nchw = nullptr;        // the output goes to the caller's NCHW memory of out_ld planes (no tensor comes back)
        int out_ld = 0;
        const UpFuse* up = nullptr;       // the caller asked upadd_fusable() first
        const ProjFuse* pj = nullptr;     // ... project_fusable()
        Tensor* pooled = nullptr;         // the output feeds a stride-2 entry: receives maxpool2(output) where the launch can write it
        GroupNormPart gn;
        int role = -1;                    // CP_ROLE_* where the shape does not say it (heads, GRU)
    };
    // What plan() makes of a ConvCall.  p is final but for the activations' addresses: every tensor the launch reads holds
    // kDryPtr (the kernel choice looks at null / non-null only), what it writes is null until conv() has allocated it.
    struct ConvPlan {
        ConvParams p;               // (with plan_split's answer: splitk, tile_m / tile_n)
        const char* err = nullptr;  // the call cannot be launched at all
        bool use16 = false;         // the f16x3 kernels take it (cp_launch_conv16), else the float32 ones
        int variant = CP_VARIANT_NONE;  // of the launch (conv_variants.h)
        bool pooled = false, up = false, pj = false;  // the requested fusion is accepted: the launch lands on a kernel that has it
    };
    // a Tensor of that shape and no memory: what a predicate hands plan() for a tensor that does not exist yet
    static Tensor shape_of(int C, int H, int W) { Tensor t; t.C = C; t.H = H; t.W = W; return t; }

    // deterministic split-K for launches with too few output tiles to fill 256 CUs (low-resolution layers at
    // small batch): slices write slabs, a small epilogue kernel sums them in order.  Returns the slices (1: no split) and sets
    // the launch's tile.
    int plan_split(ConvParams& p, bool use16, const ConvW& w) {
        int tiles = 0, nk = 0;
        cp_conv_geometry(p, use16, &tiles, &nk);
        // small launches of the f16x3 path run on 64 x 64 tiles (four times the workgroups per slice): a quarter of the
        // slices and of the slab bytes (slices x M x Cout x 4) for the same workgroup count, and no split at all where that
        // already gives kSplitTiles workgroups.  CP_SEL_TILE128_SMALL: the 128-row tiles everywhere (A/B runs).
        // Measured at B = 1 / 2 / 4 / 8 (profiles/NOTES.md): pays up to 32 tiles of 128 rows, up to 64 when K is short.
        if (use16 && tiles > 0 && (tiles <= 32 || (tiles <= 64 && nk <= 36)) && nk >= 8 && !p.gn_stats && !p.gn_in_a &&
            p.CoutPad % 64 == 0 && w.Cout >= 64 && !(g_dbg & CP_SEL_TILE128_SMALL)) {
            p.tile_m = p.tile_n = 64;
            cp_conv_geometry(p, use16, &tiles, &nk);
        }
        // (64 x 64 tiles are a quarter of the work each: they are still cut along K below one workgroup per CU)
        // (CP_SEL_STRM16_ALWAYS -- tests: the row-streaming kernel at any size -- keeps such a layer whole)
        const bool force_strm = use16 && (g_dbg & CP_SEL_STRM16_ALWAYS) && cp_strm16_supported(p);
        if (tiles > 0 && tiles < (p.tile_m == 64 ? 256 : kSplitTiles) && nk >= 8 && !p.gn_stats && !force_strm) {
            int want = (kSplitTarget + tiles - 1) / tiles;
            if (want > nk / 2) want = nk / 2;
            if (want > 32) want = 32;
            if (want > 1) {
                const int per = (nk + want - 1) / want;
                const int sk = (nk + per - 1) / per;
                if (sk > 1) return sk;
            }
        }
        return 1;
    }

    // The one place a generic conv's ConvParams is assembled and its kernel chosen: a function of the call's shapes and weights, the
    // model's precision, the switches and the dry form.  It allocates nothing and reads no activation, so conv() and the
    // predicates below -- which ask about a launch before its tensors exist -- get the same answer from the same code.
    ConvPlan plan(const ConvCall& c) {
        const ConvW& w = c.w;
        const Tensor& x0 = *c.srcs[0];
        const int nsrc = (int)c.srcs.size();
        const float* src[CP_MAX_SRC];
        int src_c[CP_MAX_SRC];
        const unsigned* src_amax[CP_MAX_SRC];
        for (int i = 0; i < nsrc; ++i) {
            src[i] = kDryPtr;
            src_c[i] = c.srcs[i]->C;
            src_amax[i] = c.srcs[i]->amax;
        }
        ConvPlan pl{conv_params(B, x0.H, x0.W, src, src_c, nsrc, w, c.stride, c.pad, c.act)};
        ConvParams& p = pl.p;
        if (p.Cin != w.CinP) {
            pl.err = "conv: channel mismatch";
            return pl;
        }
        p.res = c.res ? kDryPtr : nullptr;
        p.res_ld = c.res ? c.res->C : 0;
        p.act_from = c.act_from;
        p.offmask = c.offmask ? kDryPtr : nullptr;
        p.gn_stats = c.gn.stats_out;
        p.gn_groups = 32;
        p.gn_cpg = w.Cout / 32 > 0 ? w.Cout / 32 : 1;
        p.gn_in_a = c.gn.a;
        p.gn_in_d = c.gn.a ? c.gn.d : nullptr;
        if (c.gn.mr) {
            p.gn_in_mr = c.gn.mr; p.gn_in_gamma = c.gn.gamma; p.gn_in_beta = c.gn.beta;
            p.gn_cpg = w.Cin / 32;
        }
        pl.use16 = conv_params_f16(p, w, src_amax, m->precision == CP_PREC_F16X3);
        if (pl.use16 && p.gn_in_a) p.in_amax[0] = c.gn.bound;
        if (p.gn_in_a && !pl.use16) {  // the per-channel affine form only exists in the f16x3 1x1 kernel
            pl.err = "conv: GroupNorm affine input without an f16x3 kernel";
            return pl;
        }
        // offset/mask maps keep their padded width so the DCN loader can index [pixel*32 + c]
        p.store = c.out_nchw ? CP_STORE_NCHW : CP_STORE_NHWC;
        p.ldo = c.out_nchw ? c.out_ld : c.act == CP_ACT_SIGMOID_FROM ? w.CoutPad : w.Cout;
        p.splitk = plan_split(p, pl.use16, w);
        const bool whole16 = pl.use16 && p.splitk == 1;
        if (c.up) {
            p.up_t = kDryPtr; p.up_wt = c.up->wt; p.up_ld = c.up->t->C; p.up_f = c.up->f;
        }
        if (c.pj) {
            p.pj_src = kDryPtr; p.pj_c = c.pj->bottom->C; p.pj_amax = c.pj->bottom->amax;
            p.pj_w_hi = c.pj->w->w16f_hi; p.pj_w_lo = c.pj->w->w16f_lo; p.pj_scale = c.pj->w->scale16; p.pj_shift = c.pj->w->shift;
        }
        pl.variant = pl.use16 ? cp_conv16_variant(p) : cp_conv_variant(p);
        const bool pw16 = cp_variant_is_pw16(pl.variant);
        // dcn16t's UPADD instance; halo16's PJ on the 64- / 128-wide tile with <p>.project's fragment-ordered operands; pw16s_kernel
        // over a picture of even height and a width of whole 16-pixel blocks (a whole launch each: no split-K)
        pl.up = c.up && whole16 && pl.variant == CP_VARIANT_DCN16T && cp_dcn16t_upadd_supported(p);
        pl.pj = c.pj && whole16 && c.pj->w->CoutPad == w.CoutPad && c.pj->w->Cout == w.Cout && c.pj->w->Kpad16 == p.pj_c &&
                p.pj_w_hi && p.pj_w_lo && cp_conv16_project_supported(p);
        pl.pooled = c.pooled && whole16 && !c.out_nchw && !c.up && !c.pj && !m->form.no_pooled_producer && pw16 && cp_pw16_pool_supported(p);
        return pl;
    }
    // Would the DCN `d` on the tensor u, asked to add the up-sampling by f of a tensor of t_c channels, run on the kernel that can?
    // (boundary: the site between two IDAUps, ida(): IdaNext -- the work-space query has a form that keeps only that one)
    bool upadd_fusable(const DeformW& d, const Tensor& u, int t_c, int f, bool boundary = false) {
        using Form = cp_model::DryForm;
        if (m->form.idaup == Form::IDA_NONE || (m->form.idaup == Form::IDA_BOUNDARY && !boundary)) return false;
        const Tensor om = shape_of(32, u.H, u.W), t = shape_of(t_c, u.H / f, u.W / f);
        const UpFuse up = {&t, kDryPtr, f};
        ConvCall c{d.main, {&u}, 1, 1, CP_ACT_RELU};  // deform()'s second call
        c.offmask = &om;
        c.up = &up;
        return plan(c).up;
    }
    // Would conv2 `w2` of a level entry's first block take the projection `wp` of `bottom` as its residual -- and would that projection,
    // launched on its own, be pw16.hip's, whose arithmetic the fused form reproduces bit for bit?  float32, split-K and 64 x 64-tile
    // launches, shapes halo16 refuses, the switches that move either layer to another kernel and a tap on any entry's `.project` all
    // keep the plain sequence (a tap unfuses every entry, not only its own: the work-space query then has two forms to run, all
    // entries fused where they can be or none).
    bool project_fusable(const ConvW& wp, const ConvW& w2, const Tensor& bottom) {
        if (m->form.project_unfused || (m->tap_name && std::strstr(m->tap_name, ".project") != nullptr)) return false;  // (every entry)
        if (g_dbg & (CP_SEL_PW16_FRAG_A | CP_SEL_PW16_NEVER)) return false;  // (the projection's kernel asked for by name)
        const ConvPlan alone = plan({wp, {&bottom}, 1, 0, CP_ACT_NONE});  // tree1()'s stand-alone call
        if (alone.err || !alone.use16 || alone.p.splitk != 1 || !cp_variant_is_pw16(alone.variant))
            return false;
        const Tensor t = shape_of(w2.CinP, bottom.H, bottom.W);  // conv1's output
        const ProjFuse pj = {&bottom, &wp};
        ConvCall c{w2, {&t}, 1, 1, CP_ACT_RELU};  // basic_block()'s second call
        c.pj = &pj;
        return plan(c).pj;
    }

    // generic conv into a fresh NHWC tensor (or into user NCHW memory: ConvCall::out_nchw): plan, allocate (output, split-K slabs,
    // pooled copy -- in this order, the dry pass stops here), patch the tensors' addresses in, launch and charge
    Tensor conv(const ConvCall& c) {
        ConvPlan pl = plan(c);
        if (!pl.err && ((c.up && !pl.up) || (c.pj && !pl.pj))) pl.err = "conv: the launch has no kernel with the epilogue asked for";
        if (pl.err) {
            chk(fail(CP_ERR_INVALID, pl.err));
            return Tensor();
        }
        ConvParams& p = pl.p;
        const ConvW& w = c.w;
        Tensor out, partial;
        if (!c.out_nchw) out = make(p.ldo, p.Ho, p.Wo);
        if (p.splitk > 1) partial = make(p.splitk * p.CoutPad, p.Ho, p.Wo);
        if (pl.pooled) {
            *c.pooled = make(p.ldo, p.Ho / 2, p.Wo / 2);
            c.pooled->amax = out.amax;  // max|maxpool(x)| <= max|x|: the output's slot is a valid bound (maxpool())
        }
        if (m->dry) return out;
        for (int i = 0; i < p.nsrc; ++i) p.src[i] = c.srcs[i]->ptr();
        p.res = c.res ? c.res->ptr() : nullptr;
        p.offmask = c.offmask ? c.offmask->ptr() : nullptr;
        p.up_t = c.up ? c.up->t->ptr() : nullptr;
        p.pj_src = c.pj ? c.pj->bottom->ptr() : nullptr;
        p.out = c.out_nchw ? c.out_nchw : out.ptr();
        p.out_amax = c.out_nchw || c.act == CP_ACT_SIGMOID_FROM ? nullptr : out.amax;  // offset/mask maps are never a GEMM operand
        p.partial = p.splitk > 1 ? partial.ptr() : nullptr;
        p.pool_out = pl.pooled ? c.pooled->ptr() : nullptr;
        auto launch = [&]() -> int {
            int rc = pl.use16 ? cp_launch_conv16(p, s) : cp_launch_conv(p, s);
            if (rc == CP_OK && p.splitk > 1) rc = cp_launch_splitk_epilogue(p, s);
            return rc;
        };
        timed([&](cp_model::ProfRec& r) {
            const Tensor& x0 = *c.srcs[0];
            r.variant = pl.variant;
            r.role = c.role >= 0 ? c.role : c.offmask ? CP_ROLE_DCN : c.act == CP_ACT_SIGMOID_FROM ? CP_ROLE_DCN_OFFSET
                     : (w.KH == 1 && w.KW == 1) ? CP_ROLE_CONV1X1 : CP_ROLE_CONV;
            const double M = (double)B * p.Ho * p.Wo;
            const int cin_real = w.Cin;  // un-padded input channels
            r.flops = 2.0 * M * w.Cout * (double)(w.KH * w.KW * cin_real + (c.pj ? c.pj->w->Cin : 0));
            // algorithmic bytes: input once + output once + weights (+ offsets/mask for DCN, + residual, or the projection's
            // input and weights in its place)
            r.bytes = 4.0 * ((double)B * x0.H * x0.W * cin_real + M * w.Cout +
                             (double)w.KH * w.KW * cin_real * w.Cout + (c.offmask ? M * 27 : 0.0) +
                             (c.res ? M * w.Cout : 0.0) + (c.up ? (double)B * c.up->t->H * c.up->t->W * w.Cout : 0.0) +
                             (c.pj ? (M + w.Cout) * (double)c.pj->w->Cin : 0.0) + (pl.pooled ? M / 4 * w.Cout : 0.0));
            r.M = (int)M; r.N = w.Cout; r.K = w.KH * w.KW * cin_real; r.kh = w.KH; r.stride = c.stride;
        }, launch);
        return out;
    }
    const ConvW& cw(const std::string& k) { return m->convs.at(k); }

    // the two convs of a prediction head as launches of their own (dlav1: GroupNorm between them, gn_stats / gn)
    Tensor head_hidden(const HeadW& hw, const Tensor& x, int act, double* gn_stats) {
        ConvCall c{hw.c0, {&x}, 1, 1, act};
        c.gn.stats_out = gn_stats;
        c.role = CP_ROLE_HEAD;
        return conv(c);
    }
    // the heads of a model without GroupNorm one by one: the fused pair where it applies (try_fused), else the two convs
    void plain_heads(const Tensor& x, float* const* head_out, int sigmoid_hm, bool try_fused) {
        for (size_t i = 0; i < m->headw.size(); ++i) {
            const HeadW& hw = m->headw[i];
            const bool sg = sigmoid_hm && (hw.name == "hm" || hw.name == "hm_hp");
            float* const out = m->dry ? kDryPtr : head_out[i];
            if (try_fused && hw.w2_hi && m->precision == CP_PREC_F16X3 && !tapped() && !(g_dbg & CP_SEL_NO_HEAD_FUSION) &&
                fused_head(hw, x, sg, out))
                continue;
            Tensor hid = head_hidden(hw, x, CP_ACT_RELU, nullptr);
            head_final(hw, hid, sg, out, GroupNormPart());
        }
    }
    void head_final(const HeadW& hw, const Tensor& hid, bool sigmoid, float* out, const GroupNormPart& gn) {
        ConvCall c{hw.c1, {&hid}, 1, 0, sigmoid ? CP_ACT_SIGMOID : CP_ACT_NONE};
        c.out_nchw = out;
        c.out_ld = hw.classes;
        c.gn = gn;
        c.role = CP_ROLE_HEAD_FINAL;
        conv(c);
    }

    Tensor maxpool(const Tensor& x) {
        Tensor o = make(x.C, x.H / 2, x.W / 2);
        o.amax = x.amax;  // max|maxpool(x)| <= max|x|: the input's slot is a valid bound
        ++m->maxpool2_launches;
        if (!m->dry) chk(cp_launch_maxpool2(x.ptr(), o.ptr(), B, x.H, x.W, x.C, s));
        return o;
    }

    // residual == nullptr: pj's projection, computed by conv2 itself
    Tensor basic_block(const std::string& p, const Tensor& x, int stride, const Tensor* residual, const ProjFuse* pj = nullptr) {
        Tensor t = conv({cw(p + ".conv1"), {&x}, stride, 1, CP_ACT_RELU});
        tap(p + ".conv1", t);
        ConvCall c2{cw(p + ".conv2"), {&t}, 1, 1, CP_ACT_RELU};
        c2.res = residual;
        c2.pj = pj;
        Tensor o = conv(c2);
        tap(p, o);
        return o;
    }

    // one-level Tree (Tree.forward with levels == 1); `bottom` may be supplied by the caller when it
    // already has maxpool(x) (the outer two-level tree needs the same tensor as a root child; x's producer wrote it: conv(), lowc())
    // pool_next: the root's output feeds a stride-2 entry (conv(): pooled)
    Tensor tree1(const std::string& p, const Tensor& x, int cin, int cout, int stride, bool level_root,
                 std::vector<const Tensor*> children, const Tensor* bottom_in = nullptr, Tensor* pool_next = nullptr) {
        Tensor bottom_own;
        const Tensor* bottom = &x;
        if (stride > 1) {
            if (bottom_in) bottom = bottom_in;
            else {
                bottom_own = maxpool(x);
                bottom = &bottom_own;
            }
            tap(p + ".bottom", *bottom);
        }
        Tensor proj;
        const Tensor* residual = bottom;
        ProjFuse pj = {bottom, nullptr};
        if (cin != cout) {
            const ConvW& wp = cw(p + ".project");
            const ConvW& w2 = cw(p + ".tree1.conv2");
            if (project_fusable(wp, w2, *bottom)) {
                pj.w = &wp;  // conv2 of the first block computes the projection of its own pixels: no tensor, no launch
                residual = nullptr;
            } else {
                proj = conv({wp, {bottom}, 1, 0, CP_ACT_NONE});
                tap(p + ".project", proj);
                residual = &proj;
            }
        }
        if (level_root) children.insert(children.begin(), bottom);
        Tensor x1 = basic_block(p + ".tree1", x, stride, residual, pj.w ? &pj : nullptr);
        proj = Tensor();
        Tensor x2 = basic_block(p + ".tree2", x1, 1, &x1);
        std::vector<const Tensor*> srcs = {&x2, &x1};
        for (auto* c : children) srcs.push_back(c);
        ConvCall root{cw(p + ".root"), srcs, 1, 0, CP_ACT_RELU};
        root.pooled = pool_next;
        Tensor o = conv(root);
        tap(p + ".root", o);
        return o;
    }
    // two-level Tree with level_root = true (base.level3 / base.level4); bottom_in: maxpool(x) where x's producer wrote it
    Tensor tree2(const std::string& p, const Tensor& x, int cin, int cout, const Tensor& bottom_in, Tensor* pool_next) {
        Tensor bottom = bottom_in.valid() ? bottom_in : maxpool(x);
        tap(p + ".bottom", bottom);
        Tensor x1 = tree1(p + ".tree1", x, cin, cout, 2, false, {}, &bottom);
        return tree1(p + ".tree2", x1, cout, cout, 1, false, {&bottom, &x1}, nullptr, pool_next);
    }

    // up: the node's epilogue adds IDAUp's next up-sampled tensor; what comes back is that sum (conv(): UpFuse)
    Tensor deform(const std::string& p, const Tensor& x, const UpFuse* up = nullptr) {
        const DeformW& d = m->deforms.at(p);
        ConvCall off{d.offset, {&x}, 1, 1, CP_ACT_SIGMOID_FROM};
        off.act_from = 18;
        Tensor om = conv(off);
        tap(p + ".offmask", om, 27);
        ConvCall main{d.main, {&x}, 1, 1, CP_ACT_RELU};
        main.offmask = &om;
        main.up = up;
        Tensor o = conv(main);
        if (!up) tap(p, o);
        return o;
    }
    Tensor upsample_add(const std::string& p, const Tensor& x, int f, const Tensor& add) {
        Tensor o = make(x.C, x.H * f, x.W * f);
        if (!m->dry)
            chk(cp_launch_upsample_add(x.ptr(), m->ups.at(p), add.ptr(), o.ptr(), B, x.H, x.W, x.C, f, o.amax, s));
        return o;
    }
    // IDAUp.forward: layers[i] = node(up(proj(layers[i])) + layers[i-1]).
    // node_dead: the caller reads none of the node outputs but the last.  From the second iteration on `add` is the previous node's
    // output, and the projections do not depend on the node chain (proj_k reads layers[i] as it came in): proj_{k+1} is then launched
    // BEFORE node_k, whose epilogue adds up(t_{k+1}) to its activated output and stores u_{k+1} directly (dcn16t.hip, UPADD) -- node_k's
    // own output is never written and the upsample_add launch of iteration k + 1 (a read of `add`, a write of u) does not exist.
    // Where the node's launch is not dcn16t's (other shapes, small launches, float32, CP_SEL_DCN16T_NEVER) or a tap names a node,
    // the sequence is the plain one.  Both forms round identically (upadd_common.h).
    // The same holds one IDAUp further out (IdaNext): where the caller reads this IDAUp's last node only as the `add` of the next
    // IDAUp's first iteration, that IDAUp's proj_1 -- whose input is final by now -- is launched before the last node here, the node
    // stores u_1 of the next IDAUp, and ida() returns it for the next call's `u_first`.  This site keeps the plain sequence only
    // where the tap names that very node (or its offset / mask map): a tap on another node leaves its output unread as before, so
    // a pass with such a tap differs from the default pass in the sites inside the IDAUps alone.
    struct IdaNext {
        std::string p;        // the next IDAUp
        const Tensor* layer;  // its layers[1] (read by its proj_1)
        int f;                // its first up-sampling factor
    };
    Tensor ida(const std::string& p, std::vector<Tensor>& layers, int startp, int endp, const std::vector<int>& up_f,
               bool node_dead = false, const IdaNext* next = nullptr, Tensor u_first = Tensor()) {
        const bool tap_on_node = m->tap_name && std::strstr(m->tap_name, ".node_") != nullptr;
        Tensor u_next = u_first;  // u of the next iteration, written by this iteration's node (the first: by the IDAUp before)
        u_first = Tensor();
        for (int i = startp + 1; i < endp; ++i) {
            const std::string k = std::to_string(i - startp);
            Tensor u = u_next;
            u_next = Tensor();
            if (!u.valid()) {
                Tensor t = deform(p + ".proj_" + k, layers[i]);
                u = upsample_add(p + ".up_" + k, t, up_f[i - startp], layers[i - 1]);
            }
            tap(p + ".up_" + k, u);
            const std::string kn = std::to_string(i + 1 - startp);
            const int fn = i + 1 < endp ? up_f[i + 1 - startp] : 0;
            const DeformW& node = m->deforms.at(p + ".node_" + k);
            if (node_dead && !tap_on_node && i + 1 < endp && m->ups_t.count(p + ".up_" + kn) &&
                upadd_fusable(node, u, m->deforms.at(p + ".proj_" + kn).main.Cout, fn)) {
                Tensor t = deform(p + ".proj_" + kn, layers[i + 1]);
                const UpFuse up = {&t, m->ups_t.at(p + ".up_" + kn), fn};
                u_next = deform(p + ".node_" + k, u, &up);
                layers[i] = Tensor();  // (dead by the caller's word)
            } else if (next && i + 1 == endp && m->ups_t.count(next->p + ".up_1") &&
                       !(m->tap_name && std::strncmp(m->tap_name, (p + ".node_" + k).c_str(), (p + ".node_" + k).size()) == 0) &&
                       upadd_fusable(node, u, m->deforms.at(next->p + ".proj_1").main.Cout, next->f, true)) {
                Tensor t = deform(next->p + ".proj_1", *next->layer);
                const UpFuse up = {&t, m->ups_t.at(next->p + ".up_1"), next->f};
                u_next = deform(p + ".node_" + k, u, &up);
                layers[i] = Tensor();  // (read by the next IDAUp's first iteration only: the caller's word)
            } else {
                layers[i] = deform(p + ".node_" + k, u);
            }
        }
        return u_next;  // valid only where the last node took `next`
    }

    // the network's first layers through lowc.hip (f16x3 mode only); returns an invalid Tensor when not applicable
    // pooled (level1): the output feeds level2's stride-2 entry; where the row-streaming kernel runs over an output of even height
    // and width it writes maxpool2(output) as well and *pooled receives it (conv(): pooled -- the same contract)
    Tensor lowc(const std::string& name, int kind, const float* in, int H, int W, int planes, const unsigned* in_amax,
                Tensor* pooled = nullptr) {
        if (m->precision != CP_PREC_F16X3 || (g_dbg & CP_SEL_NO_LOWC)) return Tensor();
        const int Ho = kind == 2 ? (H - 1) / 2 + 1 : H, Wo = kind == 2 ? (W - 1) / 2 + 1 : W;
        // level1: the row-streaming kernel (lowc1s_kernel, kind 5) from the batch at which bands of >= 8 output rows give every wave
        // slot of the chip a strip (CP_SEL_LEVEL1_ROWS_NEVER / _ALWAYS: never / at any size -- tests)
        if (kind == 2 && m->lowc.count(name + ".rows") && !(g_dbg & CP_SEL_LEVEL1_ROWS_NEVER) &&
            ((g_dbg & CP_SEL_LEVEL1_ROWS_ALWAYS) || (long)B * ((Wo + 31) / 32) * ((Ho + 7) / 8) >= 2048))
            kind = 5;
        auto it = m->lowc.find(kind == 5 ? name + ".rows" : name);
        if (it == m->lowc.end()) return Tensor();
        const ConvW& w = cw(name);
        const bool stem = kind == 0 || kind == 3;  // 3: the 8-plane stem (two groups of 4 planes)
        const bool l1 = kind == 2 || kind == 5;
        const int cout = l1 ? 32 : 16, cin = stem ? planes : 16, k = stem ? 7 : 3;
        Tensor out = make(cout, Ho, Wo);
        const bool pool = pooled && !m->form.no_pooled_producer && cp_lowc_pool_supported(kind, H, W);
        if (pool) {
            *pooled = make(cout, Ho / 2, Wo / 2);
            pooled->amax = out.amax;  // (maxpool(): the output's slot is a valid bound)
        }
        if (m->dry) return out;
        auto launch = [&]() {
            return cp_launch_lowc(kind, in, out.ptr(), it->second.hi, it->second.lo, it->second.scale16, w.shift, in_amax,
                                  out.amax, B, H, W, planes, s, pool ? pooled->ptr() : nullptr);
        };
        timed([&](cp_model::ProfRec& r) {
            r.variant = kind == 5 ? CP_VARIANT_LOWC1S : kind == 1 ? CP_VARIANT_LOWC1 : kind == 2 ? CP_VARIANT_LOWC2 : CP_VARIANT_LOWC0;  // (3: the 8-plane stem)
            r.role = CP_ROLE_LOWC;
            const double M = (double)B * Ho * Wo;
            r.flops = 2.0 * M * cout * (double)(k * k * cin);
            r.bytes = 4.0 * ((double)B * H * W * cin + M * cout + (double)k * k * cin * cout + (pool ? M / 4 * cout : 0.0));
            r.M = (int)M; r.N = cout; r.K = k * k * cin; r.kh = k; r.stride = l1 ? 2 : 1;
        }, launch);
        return out;
    }

    Tensor to_nhwc(const float* nchw, int C, int Cpad, int H, int W) {
        Tensor t = make(Cpad, H, W);
        t.amax = nullptr;  // re-laid network inputs only feed the exact-f32 stems
        if (!m->dry) chk(cp_launch_nchw_to_nhwc(nchw, t.ptr(), B, C, H, W, Cpad, s));
        return t;
    }
    // a 7x7 stem of the DLA base on a caller-owned NCHW input of C planes: the direct low-channel kernel (lowc.hip) where it
    // applies, else the input re-laid to Cpad channels + the generic conv
    Tensor stem(const char* name, int kind, const float* nchw, int H, int W, int C, int Cpad, bool use_lowc) {
        Tensor t = lowc(name, kind, nchw, H, W, C, use_lowc && !m->dry ? input_slot(nchw, (size_t)B * C * H * W) : nullptr);
        if (!t.valid()) {
            Tensor in = to_nhwc(nchw, C, Cpad, H, W);
            t = conv({cw(name), {&in}, 1, 3, CP_ACT_RELU});
        }
        return t;
    }

    // ---- stacked hourglass forward (large_hourglass.py:50-78, 129-189, 266-286) ----
    Tensor hg_residual(const std::string& p, const Tensor& x, int stride) {
        Tensor t = conv({cw(p + ".conv1"), {&x}, stride, 1, CP_ACT_RELU});
        Tensor sk;
        if (m->convs.count(p + ".skip")) sk = conv({cw(p + ".skip"), {&x}, stride, 0, CP_ACT_NONE});
        ConvCall c2{cw(p + ".conv2"), {&t}, 1, 1, CP_ACT_RELU};
        c2.res = sk.valid() ? &sk : &x;  // relu(bn2(conv2) + skip)
        return conv(c2);
    }
    Tensor hg_seq(const std::string& p, Tensor x, int n, int first_stride) {
        for (int i = 0; i < n; ++i) x = hg_residual(p + "." + std::to_string(i), x, i == 0 ? first_stride : 1);
        return x;
    }
    Tensor hg_kp(const std::string& p, const Tensor& x, int n, const int* mods) {
        const int cm = mods[0], nm = mods[1];
        Tensor up1 = hg_seq(p + ".up1", x, cm, 1);
        Tensor low = hg_seq(p + ".low1", x, cm, 2);
        low = n > 1 ? hg_kp(p + ".low2", low, n - 1, mods + 1) : hg_seq(p + ".low2", low, nm, 1);
        low = hg_seq(p + ".low3", low, cm, 1);
        Tensor out = make(up1.C, up1.H, up1.W);
        if (!m->dry)
            chk(cp_launch_upsample2_nearest_add(up1.ptr(), low.ptr(), out.ptr(), B, low.H, low.W, low.C, out.amax, s));
        tap(p, out);
        return out;
    }
    void run_hourglass(int H, int W, const float* images, float* const* head_out, int sigmoid_hm) {
        static const int mods[6] = {2, 2, 2, 2, 2, 4};
        init_slots();
        Tensor inter;
        {
            Tensor in = to_nhwc(images, 3, 4, H, W);
            Tensor p0 = conv({cw("pre.0"), {&in}, 2, 3, CP_ACT_RELU});
            inter = hg_residual("pre.1", p0, 2);
        }
        tap("pre", inter);
        Tensor cnv;
        for (int k = 0; k < 2; ++k) {
            const std::string ks = std::to_string(k);
            Tensor kp = hg_kp("kps." + ks, inter, 5, mods);
            cnv = conv({cw("cnvs." + ks), {&kp}, 1, 1, CP_ACT_RELU});
            tap("cnvs." + ks, cnv);
            if (k == 0) {
                Tensor a = conv({cw("inters_.0"), {&inter}, 1, 0, CP_ACT_NONE});
                ConvCall cb{cw("cnvs_.0"), {&cnv}, 1, 0, CP_ACT_RELU};
                cb.res = &a;  // relu(inters_(inter) + cnvs_(cnv))
                Tensor b = conv(cb);
                inter = hg_residual("inters.0", b, 1);
            }
        }
        if (fused_heads_grouped(cnv, head_out, sigmoid_hm)) return;
        plain_heads(cnv, head_out, sigmoid_hm, true);
    }

    // ---- PoseResNet forward (resnet_dcn.py: PoseResNet.forward, BasicBlock / Bottleneck.forward) ----
    Tensor deconv(const std::string& p, const Tensor& x) {
        const DeconvW& d = m->deconvs.at(p);
        Tensor o = make(d.Cout, 2 * x.H, 2 * x.W);
        if (m->dry) return o;
        if (x.C != d.Cin) {
            chk(fail(CP_ERR_INVALID, "deconv: channel mismatch"));
            return o;
        }
        const DeconvLaunch l = deconv_launch(d, m->precision == CP_PREC_F16X3, x.ptr(), x.amax, B, x.H, x.W, o.ptr(), o.amax, true);
        timed([&](cp_model::ProfRec& r) {
            r.variant = l.f16x3 ? CP_VARIANT_DECONV16 : CP_VARIANT_DECONV_F32;
            r.role = CP_ROLE_DECONV;
            const double M = (double)B * x.H * x.W;  // rows of one sub-pixel class
            r.flops = 2.0 * 4 * M * d.Cout * 4.0 * d.Cin;
            r.bytes = 4.0 * (M * d.Cin + 4 * M * d.Cout + 16.0 * d.Cin * d.Cout);
            r.M = (int)(4 * M); r.N = d.Cout; r.K = 4 * d.Cin; r.kh = 4; r.stride = 2;
        }, [&]() { return cp_launch_deconv(l, s); });
        return o;
    }
    Tensor maxpool3(const Tensor& x) {
        Tensor o = make(x.C, (x.H - 1) / 2 + 1, (x.W - 1) / 2 + 1);
        if (!m->dry) chk(cp_launch_maxpool3s2(x.ptr(), o.ptr(), B, x.H, x.W, x.C, o.amax, s));
        return o;
    }
    Tensor res_block(const std::string& p, const Tensor& x, int stride, bool bott) {
        Tensor sk;
        const Tensor* res = &x;
        if (m->convs.count(p + ".downsample")) {
            sk = conv({cw(p + ".downsample"), {&x}, stride, 0, CP_ACT_NONE});
            res = &sk;
        }
        Tensor a, b;
        if (bott) {
            a = conv({cw(p + ".conv1"), {&x}, 1, 0, CP_ACT_RELU});
            b = conv({cw(p + ".conv2"), {&a}, stride, 1, CP_ACT_RELU});
            a = Tensor();
        } else {
            b = conv({cw(p + ".conv1"), {&x}, stride, 1, CP_ACT_RELU});
        }
        ConvCall last{cw(p + (bott ? ".conv3" : ".conv2")), {&b}, 1, bott ? 0 : 1, CP_ACT_RELU};
        last.res = res;  // relu(bn(conv) + residual)
        return conv(last);
    }
    void run_resnet(int H, int W, const float* images, float* const* head_out, int sigmoid_hm) {
        bool bott = false;
        int blocks[4] = {0, 0, 0, 0};
        resnet_spec(m->resnet, &bott, blocks);
        init_slots();
        Tensor x;
        {
            Tensor in = to_nhwc(images, 3, 4, H, W);
            Tensor c1 = conv({cw("conv1"), {&in}, 2, 3, CP_ACT_RELU});
            in = Tensor();
            x = maxpool3(c1);
        }
        tap("maxpool", x);
        for (int l = 0; l < 4; ++l) {
            const std::string ln = "layer" + std::to_string(l + 1);
            for (int b = 0; b < blocks[l]; ++b) x = res_block(ln + "." + std::to_string(b), x, b == 0 && l ? 2 : 1, bott);
            tap(ln, x);
        }
        for (int i = 0; i < 3; ++i) {
            const std::string fc = "deconv_layers." + std::to_string(6 * i);
            x = deform(fc, x);
            tap("deconv_layers." + std::to_string(6 * i + 2), x);
            x = deconv("deconv_layers." + std::to_string(6 * i + 3), x);
            tap("deconv_layers." + std::to_string(6 * i + 5), x);
        }
        if (features_only(x)) return;
        plain_heads(x, head_out, sigmoid_hm, false);
    }

    void run(int H, int W, const float* images, const float* pre_img, const float* pre_hm, const float* pre_hm_hp,
             float* const* head_out, int sigmoid_hm) {
        init_slots();
        const bool use_lowc = m->precision == CP_PREC_F16X3 && !(g_dbg & CP_SEL_NO_LOWC) && m->lowc.count("base.base_layer");
        // stem + level0 in one launch when nothing is added to the stem's output (no previous-frame stems) and nobody asks for it
        // (CP_SEL_STEM_LEVEL0_UNFUSED: the two kernels, A/B runs and tests)
        const bool no_pre = m->dry ? m->form.stem_level0_fused : (!pre_img && !pre_hm && !pre_hm_hp);
        const bool fuse01 = use_lowc && no_pre && m->lowc.count("base.level0.rows") && m->stem_bound_l > 0.f &&
                            !(g_dbg & CP_SEL_STEM_LEVEL0_UNFUSED) && !(m->tap_name && std::strcmp(m->tap_name, "base.base_layer") == 0) &&
                            !m->convs.count("base.pre_img_layer") && !m->convs.count("base.pre_hm_layer") && !m->convs.count("base.pre_hm_hp_layer");
        Tensor l0f;
        if (fuse01) {
            const unsigned* in_slot = !m->dry ? input_slot(images, (size_t)B * 3 * H * W) : nullptr;
            l0f = make(16, H, W);
            if (!m->dry) {
                const LowcW& a = m->lowc["base.base_layer"];
                const LowcW& c = m->lowc["base.level0.rows"];
                auto launch = [&]() {
                    return cp_launch_lowc_fused(images, l0f.ptr(), a.hi, a.lo, a.scale16, cw("base.base_layer").shift, c.hi, c.lo, c.scale16,
                                                cw("base.level0").shift, m->stem_bound_l, m->stem_bound_s, in_slot, l0f.amax, B, H, W, 3, s);
                };
                timed([&](cp_model::ProfRec& r) {
                    r.variant = CP_VARIANT_LOWC01;
                    r.role = CP_ROLE_LOWC;
                    const double M = (double)B * H * W;
                    r.flops = 2.0 * M * 16 * (147.0 + 144.0);
                    r.bytes = 4.0 * (M * 3 + M * 16);
                    r.M = (int)M; r.N = 16; r.K = 147 + 144; r.kh = 7; r.stride = 1;
                }, launch);
            }
        }
        Tensor x0 = fuse01 ? Tensor() : stem("base.base_layer", 0, images, H, W, 3, 4, use_lowc);
        // a dry run (workspace query) is sized for every stem the model has
        if (m->dry) {
            if (!m->convs.count("base.pre_img_layer")) pre_img = nullptr;
            if (!m->convs.count("base.pre_hm_layer")) pre_hm = nullptr;
            if (!m->convs.count("base.pre_hm_hp_layer")) pre_hm_hp = nullptr;
        }
        if ((pre_img && !m->convs.count("base.pre_img_layer")) || (pre_hm && !m->convs.count("base.pre_hm_layer")) ||
            (pre_hm_hp && !m->convs.count("base.pre_hm_hp_layer"))) {
            chk(fail(CP_ERR_INVALID, "a previous-frame input was given to a model built without that pre_* layer"));
            return;
        }
        if (pre_img || pre_hm || pre_hm_hp) {
            Tensor a, b, c;
            if (pre_img) a = stem("base.pre_img_layer", 0, pre_img, H, W, 3, 4, use_lowc);
            if (pre_hm) b = stem("base.pre_hm_layer", 0, pre_hm, H, W, 1, 4, use_lowc);
            if (pre_hm_hp) c = stem("base.pre_hm_hp_layer", 3, pre_hm_hp, H, W, 8, 8, use_lowc);
            // x = x + pre_img_layer(..) + pre_hm_layer(..) + pre_hm_hp_layer(..)  (left-to-right, :312-318)
            std::vector<const Tensor*> adds;
            for (Tensor* t : {&a, &b, &c})
                if (t->valid()) adds.push_back(t);
            Tensor sum = make(16, H, W);
            if (!m->dry)
                chk(cp_launch_add_relu_sum(x0.ptr(), adds[0]->ptr(), adds.size() > 1 ? adds[1]->ptr() : nullptr,
                                           adds.size() > 2 ? adds[2]->ptr() : nullptr, sum.ptr(),
                                           (size_t)B * H * W * 16, sum.amax, s));
            x0 = sum;
        }
        if (!fuse01) tap("base.base_layer", x0);
        Tensor l0 = fuse01 ? l0f : lowc("base.level0", 1, x0.ptr(), H, W, 16, x0.amax);
        l0f = Tensor();  // (one owner: the block returns to the arena when l0 is dropped below)
        if (!l0.valid()) l0 = conv({cw("base.level0"), {&x0}, 1, 1, CP_ACT_RELU});
        tap("base.level0", l0);
        x0 = Tensor();
        // the 2x2 max-pooled copy each stride-2 entry reads (Tree.downsample), written by the launch that produces the entry's
        // input where it can (lowc(), conv(): pooled); an invalid one makes the entry launch maxpool2
        Tensor pl[4];
        Tensor l1 = lowc("base.level1", 2, l0.ptr(), H, W, 16, l0.amax, &pl[0]);
        if (!l1.valid()) l1 = conv({cw("base.level1"), {&l0}, 2, 1, CP_ACT_RELU});
        tap("base.level1", l1);
        l0 = Tensor();
        std::vector<Tensor> L(6);
        L[2] = tree1("base.level2", l1, 32, 64, 2, false, {}, pl[0].valid() ? &pl[0] : nullptr, &pl[1]);
        l1 = pl[0] = Tensor();
        L[3] = tree2("base.level3", L[2], 64, 128, pl[1], &pl[2]);
        pl[1] = Tensor();
        L[4] = tree2("base.level4", L[3], 128, 256, pl[2], &pl[3]);
        pl[2] = Tensor();
        L[5] = tree1("base.level5", L[4], 256, 512, 2, true, {}, pl[3].valid() ? &pl[3] : nullptr);
        pl[3] = Tensor();
        tap("base.level2", L[2]);
        tap("base.level3", L[3]);
        tap("base.level4", L[4]);
        tap("base.level5", L[5]);

        // DLAUp.forward (:437-443): out = [after ida_2, after ida_1, after ida_0, L5]
        ida("dla_up.ida_0", L, 4, 6, {1, 2});
        Tensor o2 = L[5];  // 256 @ 1/8... (after ida_0: 256 ch at L4 resolution)
        ida("dla_up.ida_1", L, 3, 6, {1, 2, 2});
        Tensor o1 = L[5];
        // (only L[5] is read below, and only as the `add` of ida_up's first iteration: where the last node can, it stores that
        // iteration's u instead and o0 does not exist)
        const IdaNext to_ida_up = {"ida_up", &o1, 2};
        Tensor u1 = ida("dla_up.ida_2", L, 2, 6, {1, 2, 2, 2}, true, &to_ida_up);
        Tensor o0 = L[5];
        for (auto& t : L) t = Tensor();
        // DLASeg.forward (:531-536): ida_up over [o0, o1, o2]
        std::vector<Tensor> y = {o0, o1, o2};
        o0 = o1 = o2 = Tensor();
        ida("ida_up", y, 0, 3, {1, 2, 4}, true, nullptr, u1);  // (only y[2] is read below)
        u1 = Tensor();
        Tensor feat = y[2];
        y.clear();
        tap("feat", feat);
        if (features_only(feat)) return;

        std::vector<Tensor> gru_out;
        if (m->gru) {
            const int steps = m->tracking ? 4 : 3;
            ConvCall cx{m->gru_x, {&feat}, 1, 1, CP_ACT_NONE};
            cx.role = CP_ROLE_GRU;
            Tensor x3 = conv(cx);
            Tensor h;
            for (int st = 0; st < steps; ++st) {
                Tensor hn = make(64, feat.H, feat.W);
                const size_t M = (size_t)B * feat.H * feat.W;
                if (st == 0) {
                    // h0 = 0: the three hidden-side convolutions are identically zero (convGRU.py:51,80-84)
                    if (!m->dry) chk(cp_launch_gru_gate(x3.ptr(), nullptr, nullptr, hn.ptr(), M, hn.amax, s));
                } else if (m->precision == CP_PREC_F16X3 && m->gru_h16_hi && !(g_dbg & CP_SEL_GRU_UNFUSED) &&
                           (size_t)M * 192 * 4 < (size_t)0xf0000000u) {
                    // hidden-side convolution with the gate arithmetic in its epilogue: h3 is never written
                    if (!m->dry) {
                        ConvW w;  // the three hidden-side 3x3 layers in fused-gate order: f16x3 operands only, no affine
                        w.KH = w.KW = 3;
                        w.K = w.Kpad = w.Kpad16 = 576;
                        w.Cout = w.CoutPad = 192;
                        w.w16_hi = m->gru_h16_hi;
                        w.w16_lo = m->gru_h16_lo;
                        w.w16f_hi = m->gru_h16f_hi;
                        w.w16f_lo = m->gru_h16f_lo;
                        w.scale16 = m->gru_h16_inv;  // 2^-e of the fused-order weight rows
                        const float* src = h.ptr();
                        ConvParams p = conv_params(B, feat.H, feat.W, &src, &h.C, 1, w, 1, 1, CP_ACT_NONE);
                        conv_params_f16(p, w, &h.amax, true, true);
                        p.out_amax = hn.amax;
                        p.out = hn.ptr();
                        p.gru_x3 = x3.ptr();
                        p.gru_hprev = h.ptr();
                        p.splitk = 1;
                        timed([&](cp_model::ProfRec& r) {
                            r.variant = cp_conv16_gru_variant(p);
                            r.role = CP_ROLE_GRU;
                            r.flops = 2.0 * (double)M * 192 * 576;
                            r.bytes = 4.0 * ((double)M * (64 + 192 + 64 + 64) + 576.0 * 192);
                            r.M = (int)M; r.N = 192; r.K = 576; r.kh = 3; r.stride = 1;
                        }, [&]() { return cp_launch_conv16_gru(p, s); });
                    }
                } else {
                    ConvCall ch{m->gru_h, {&h}, 1, 1, CP_ACT_NONE};
                    ch.role = CP_ROLE_GRU;
                    Tensor h3 = conv(ch);
                    if (!m->dry) chk(cp_launch_gru_gate(x3.ptr(), h3.ptr(), h.ptr(), hn.ptr(), M, hn.amax, s));
                }
                h = hn;
                gru_out.push_back(h);
                tap(("convGRU.step" + std::to_string(st)).c_str(), h);
            }
        }

        if (!m->gru) {
            if (!fused_heads_grouped(feat, head_out, sigmoid_hm)) plain_heads(feat, head_out, sigmoid_hm, true);
            return;
        }
        // dlav1: conv3x3 -> GroupNorm -> ReLU -> conv1x1 on the head's ConvGRU step.  GroupNorm statistics of every head (32 groups x
        // (sum, sumsq) doubles per image = 128 floats per image and head): one block, zeroed by one memset per forward pass
        Tensor stats_all = make(128 * (int)m->headw.size(), 1, 1);
        if (!m->dry && hipMemsetAsync(stats_all.ptr(), 0, sizeof(double) * 64 * B * m->headw.size(), s) != hipSuccess) chk(CP_ERR_LAUNCH);
        for (size_t i = 0; i < m->headw.size(); ++i) {
            const HeadW& hw = m->headw[i];
            int r = -1;
            const std::string& n = hw.name;
            if (m->tracking) {
                if (n == "tracking" || n == "tracking_hp") r = 0;
                else if (n == "hm" || n == "wh" || n == "reg") r = 1;
                else if (n == "hm_hp" || n == "hp_offset" || n == "hps" || n == "hps_uncertainty") r = 2;
                else if (n == "scale" || n == "scale_uncertainty") r = 3;
            } else {
                if (n == "hm" || n == "wh" || n == "reg") r = 0;
                else if (n == "hm_hp" || n == "hp_offset" || n == "hps") r = 1;
                else if (n == "scale") r = 2;
            }
            if (r < 0) {  // unreachable: cp_model_create refuses heads outside the routing table
                chk(fail(CP_ERR_STATE, "head without a ConvGRU step"));
                continue;
            }
            const Tensor* src = &gru_out[r];
            Tensor mr = make(64, 1, 1), ad;
            double* stats = !m->dry ? (double*)stats_all.ptr() + (size_t)i * 64 * B : nullptr;
            const bool fuse_gn = ((src->H * src->W) % 32 == 0) && hw.c0.Cout % 32 == 0 && (hw.c0.Cout / 32) % 4 == 0;
            const bool sg = sigmoid_hm && (hw.name == "hm" || hw.name == "hm_hp");
            // KEPT DIVERGENCE: the GroupNorm parts (`stats` here, gn below) only exist in a real pass, so the dry pass plans both
            // convs without them: it may plan split-K slabs the real pass does not have, and it sends the final 1x1 through conv()
            // where the real pass runs gn_final.  It over-estimates, which is safe.  (Handing the dry pass kDryPtr in their place
            // makes the two agree, and changes what cp_model_workspace_bytes returns for dlav1.)
            Tensor hid = head_hidden(hw, *src, CP_ACT_NONE, fuse_gn && !m->dry ? stats : nullptr);
            GroupNormPart gn;
            if (fuse_gn) {
                // statistics came out of the conv epilogue; normalise + affine + ReLU happens in the 1x1 loader
                const bool affine16 = m->precision == CP_PREC_F16X3 && hw.c1.w16_hi && (hid.H * hid.W) % 128 == 0 &&
                                      !(g_dbg & CP_SEL_GN_HEAD_F32);
                if (affine16) {
                    // f16x3 1x1 kernel: the normalisation pre-folded to y = relu(a*x + d) per (image, channel)
                    ad = make(2 * hid.C, 1, 1);
                    if (!m->dry) {
                        float* ap = ad.ptr();
                        float* dp = ap + (size_t)B * hid.C;
                        unsigned* bound = new_slot();
                        chk(cp_launch_gn_affine((const double*)stats, hw.gn_gamma, hw.gn_beta, ap, dp, B, hid.C, 32,
                                                (double)hid.H * hid.W * (hid.C / 32), 1e-5f, hid.amax, bound, s));
                        gn.a = ap; gn.d = dp; gn.bound = bound;
                    }
                } else if (!m->dry) {
                    chk(cp_launch_gn_finalize((const double*)stats, mr.ptr(), B * 32, (double)hid.H * hid.W * (hid.C / 32), 1e-5f, s));
                    gn.mr = mr.ptr(); gn.gamma = hw.gn_gamma; gn.beta = hw.gn_beta;
                }
            } else if (!m->dry) {
                // in place: the slot keeps the larger of the raw and the normalised |max| -- a valid bound
                chk(cp_launch_groupnorm_relu(hid.ptr(), hw.gn_gamma, hw.gn_beta, stats, B, hid.H * hid.W, hid.C, 32, 1e-5f, hid.amax, s));
            }
            if (gn.a && !(g_dbg & CP_SEL_GN_HEAD_MFMA) && hid.C % 64 == 0 && hid.C <= 256 && (hid.H * hid.W) % 64 == 0 &&
                ((size_t)B * hid.H * hid.W) % 256 == 0 && hw.classes <= 16 && !tapped()) {
                // float32 vector-ALU kernel (ewise.hip: gn_final_kernel): the layer is an HBM stream of the hidden tensor
                auto launch = [&]() -> int {
                    return cp_launch_gn_final(hid.ptr(), gn.a, gn.d, hw.c1.wp, hw.c1.shift, head_out[i], B, hid.H * hid.W,
                                              hid.C, hw.classes, hw.c1.CoutPad, sg ? 1 : 0, s);
                };
                timed([&](cp_model::ProfRec& r) {
                    r.variant = CP_VARIANT_GN_FINAL;
                    r.role = CP_ROLE_HEAD_FINAL;
                    const double M = (double)B * hid.H * hid.W;
                    r.flops = 2.0 * M * hw.classes * (double)hid.C;
                    r.bytes = 4.0 * (M * hid.C + M * hw.classes + (double)hid.C * hw.classes);
                    r.M = (int)M; r.N = hw.classes; r.K = hid.C; r.kh = 1; r.stride = 1;
                }, launch);
                continue;
            }
            head_final(hw, hid, sg, m->dry ? kDryPtr : head_out[i], gn);
        }
    }
};

}  // namespace

int cp_engine::forward_impl(cp_model* m, hipStream_t stream, int B, int H, int W, const float* images, const float* pre_img,
                 const float* pre_hm, const float* pre_hm_hp, float* const* head_out, int sigmoid_hm, void* ws,
                 size_t ws_bytes, bool dry) {
    if (!m || !m->finalized) return fail(CP_ERR_STATE, "model not finalized");
    if (B < 1 || H % 32 || W % 32 || H < 32 || W < 32) return fail(CP_ERR_INVALID, "H and W must be multiples of 32");
    if (m->hourglass && (H % 128 || W % 128))
        return fail(CP_ERR_INVALID, "hourglass: H and W must be multiples of 128 (stride 4, then five stride-2 levels)");
    m->arena.reset(dry ? nullptr : ws, ws_bytes);
    m->dry = dry;
    m->status = CP_OK;
    m->maxpool2_launches = 0;
    Fwd f{m, B, stream};
    if (m->hourglass) f.run_hourglass(H, W, images, head_out, sigmoid_hm);
    else if (m->resnet) f.run_resnet(H, W, images, head_out, sigmoid_hm);
    else f.run(H, W, images, pre_img, pre_hm, pre_hm_hp, head_out, sigmoid_hm);
    if (!dry && m->arena.overflow)
        return fail(CP_ERR_INVALID, "workspace too small: " + std::to_string(ws_bytes) + " bytes given, this launch sequence peaks at " +
                                        std::to_string(m->arena.peak));
    return m->status;
}

// the heads of group g on the feature map the last lean detect kept (cp_model_dense_heads)
int cp_engine::kept_dense_heads(cp_model* m, hipStream_t stream, float* const* head_out) {
    const auto& k = m->kept;
    m->dry = false;
    m->status = CP_OK;
    Fwd f{m, k.B, stream};
    if (!lean_finished_maps(m) && !k.slabs)
        return fail(CP_ERR_STATE, "dense heads: the lean detect's workspace was sized without room for the slabs this switch setting needs");
    if (!f.grouped_launch(m->reg_group, k.ptr, k.amax, k.C, k.H, k.W, head_out, 0, k.slabs))
        return fail(CP_ERR_STATE, "dense heads: the grouped head launch does not apply under the current switches");
    return m->status;
}

// every regression head at caller-given pixels of the kept feature map (cp_model_heads_at)
int cp_engine::kept_heads_at(cp_model* m, hipStream_t stream, const int* index, int n, float* const* table_out, float* slabs) {
    const auto& k = m->kept;
    m->dry = false;
    m->status = CP_OK;
    Fwd f{m, k.B, stream};
    f.heads_at_rows(0, (int)m->reg_group.idx.size(), k.ptr, k.amax, k.C, k.H, k.W, index, n, n, k.B, n, table_out, slabs);
    return m->status;
}
