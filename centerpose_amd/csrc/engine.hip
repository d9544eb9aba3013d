// The model's run-time C ABI (include/centerpose_hip.h): forward / detect / tap / profile / precision / debug, and the
// one-line wrappers of the other modules (decode, post-process, PnP, tracking, box metrics, pose loss, pose targets).
// Host-side C++ only orchestrates: parameters are folded / packed once at cp_model_finalize (engine_pack.hip), the forward
// pass is a fixed sequence of HIP kernel launches (engine_forward.hip); the stand-alone operators live in ops.hip.
#include "engine_model.h"
#include "track_common.h"

namespace {
thread_local std::string g_err;  // cp_last_error(): per calling thread
}

namespace cp_engine {
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int g_default_precision = CP_PREC_F32;
int g_dbg = 0;
}  // namespace cp_engine

using namespace cp_engine;

// a call that is about to write `ws`: the feature map a lean detect left in it (cp_model::kept) is gone
static void drop_kept_in(cp_model* m, const void* ws, size_t bytes) {
    const char* k = (const char*)m->kept.ptr;
    if (k && k >= (const char*)ws && k < (const char*)ws + bytes) m->kept = cp_model::KeptFeat();
}

// The gate in front of a pass that allocates from the caller's workspace: nothing is launched on a workspace smaller than the query's
// answer for this (shape, switches, precision).  Arena::alloc hands out offsets beyond its cap and only notes the overflow, which
// forward_impl reports once every launch is enqueued: without this gate a buffer sized for another arithmetic mode or switch setting
// is written past its end.  (The query is cached per shape and switches and dropped by cp_model_set_precision: a compare.)
static int workspace_refused(cp_model* m, const char* what, int B, int H, int W, size_t workspace_bytes) {
    if (!m) return fail(CP_ERR_INVALID, std::string(what) + ": null model");
    if (!m->finalized) return fail(CP_ERR_STATE, "model not finalized");
    const size_t need = cp_model_workspace_bytes(m, B, H, W);
    if (need == 0) return CP_ERR_INVALID;  // (the shape was refused: the dry pass left the reason in cp_last_error)
    if (workspace_bytes < need)
        return fail(CP_ERR_INVALID, std::string(what) + ": workspace too small: " + std::to_string(workspace_bytes) +
                                        " bytes given, cp_model_workspace_bytes asks for " + std::to_string(need));
    return CP_OK;
}

// captured launch sequences of a model, keyed by every argument: replay the graph of `key`, capturing `enqueue` on first use
template <class F>
static int replay_or_capture(cp_model* m, hipStream_t s, const std::vector<uint64_t>& key, F&& enqueue) {
    auto it = m->graphs.find(key);
    if (it == m->graphs.end()) {
        if (s == nullptr) return fail(CP_ERR_INVALID, "graph capture needs a non-default stream");
        if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess)
            return fail(CP_ERR_LAUNCH, "hipStreamBeginCapture failed");
        const int rc = enqueue();
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(s, &g);
        if (rc != CP_OK || e != hipSuccess || !g) {
            if (g) (void)hipGraphDestroy(g);
            return rc != CP_OK ? rc : fail(CP_ERR_LAUNCH, "hipStreamEndCapture failed");
        }
        hipGraphExec_t ex = nullptr;
        if (hipGraphInstantiate(&ex, g, nullptr, nullptr, 0) != hipSuccess) {
            (void)hipGraphDestroy(g);
            return fail(CP_ERR_LAUNCH, "hipGraphInstantiate failed");
        }
        (void)hipGraphDestroy(g);
        if (m->graphs.size() >= 16) {  // bound the cache
            for (auto& kv : m->graphs) (void)hipGraphExecDestroy(kv.second);
            m->graphs.clear();
            m->graph_kept.clear();
        }
        it = m->graphs.emplace(key, ex).first;
    }
    return hipGraphLaunch(it->second, s) == hipSuccess ? CP_OK : fail(CP_ERR_LAUNCH, "hipGraphLaunch failed");
}


// ============================================ C ABI ==============================================
extern "C" {

const char* cp_version(void) { return "centerpose_hip 0.3.0 (gfx950; f32 and split-f16 MFMA)"; }
int cp_abi_version(void) { return CP_ABI_VERSION; }
static_assert(CP_NUM_KERNEL_VARIANTS == CP_NUM_CONV_VARIANTS, "public and internal kernel-variant counts");
int cp_num_kernel_variants(void) { return CP_NUM_KERNEL_VARIANTS; }
int cp_num_roles(void) { return CP_NUM_ROLES; }
const char* cp_last_error(void) { return g_err.c_str(); }

int cp_set_debug(int flags) {
    // a bit outside CP_SEL_ALL (unknown, or a retired switch) is refused rather than reinterpreted
    if (flags & ~CP_SEL_ALL)
        return fail(CP_ERR_INVALID, "cp_set_debug: unknown switch bits " + std::to_string(flags & ~CP_SEL_ALL));
    g_dbg = flags;
    return CP_OK;
}

int cp_set_default_precision(int precision) {
    if (precision != CP_PREC_F32 && precision != CP_PREC_F16X3) return fail(CP_ERR_INVALID, "precision must be 0 or 1");
    g_default_precision = precision;
    return CP_OK;
}

int cp_model_set_precision(cp_model* m, int precision) {
    if (!m || (precision != CP_PREC_F32 && precision != CP_PREC_F16X3)) return fail(CP_ERR_INVALID, "bad argument");
    m->precision = precision;
    m->ws_cached = 0;  // (the two arithmetic modes run different launch sequences)
    return CP_OK;
}

int cp_model_profile(cp_model* m, int enable) {
    if (!m) return fail(CP_ERR_INVALID, "null model");
    m->profile = enable != 0;
    return CP_OK;
}

// Drains the recorded launches (synchronises their events).  out[v*4 + {0,1,2,3}] = {launches, total ms,
// total algorithmic FLOPs, total algorithmic bytes} for kernel variant v (names: cp_conv_variant_name).
int cp_model_profile_read(cp_model* m, double* out, int num_variants) {
    if (!m || !out || num_variants < CP_NUM_CONV_VARIANTS) return fail(CP_ERR_INVALID, "bad argument");
    for (int i = 0; i < num_variants * 4; ++i) out[i] = 0.0;
    for (int i = 0; i < CP_NUM_ROLES * 4; ++i) m->roles[i] = 0.0;
    const char* dump = getenv("CP_PROFILE_DUMP");  // optional per-launch CSV for kernel tuning
    FILE* df = dump ? fopen(dump, "a") : nullptr;
    for (auto& r : m->prof) {
        float ms = 0.f;
        if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess)
            return fail(CP_ERR_LAUNCH, "event timing failed");
        if (df)
            fprintf(df, "%s,%d,%d,%d,%d,%d,%.4f,%.2f,%s\n", r.variant >= 0 ? cp_conv_variant_name(r.variant) : "decode", r.M,
                    r.N, r.K, r.kh, r.stride, ms, r.flops / (ms * 1e-3) / 1e12, cp_role_name(r.role));
        if (r.variant >= 0) {
            out[r.variant * 4 + 0] += 1.0;
            out[r.variant * 4 + 1] += ms;
            out[r.variant * 4 + 2] += r.flops;
            out[r.variant * 4 + 3] += r.bytes;
        }
        if (r.role >= 0 && r.role < CP_NUM_ROLES) {
            m->roles[r.role * 4 + 0] += 1.0;
            m->roles[r.role * 4 + 1] += ms;
            m->roles[r.role * 4 + 2] += r.flops;
            m->roles[r.role * 4 + 3] += r.bytes;
        }
        m->event_pool.push_back(r.e0);
        m->event_pool.push_back(r.e1);
    }
    m->prof.clear();
    if (df) fclose(df);
    return CP_OK;
}

const char* cp_kernel_variant_name(int v) { return cp_conv_variant_name(v); }

const char* cp_role_name(int role) {
    static const char* names[CP_NUM_ROLES] = {"conv", "conv1x1", "dcn", "dcn_offset", "head", "head_final", "gru", "lowc",
                                              "decode", "deconv"};
    return (role >= 0 && role < CP_NUM_ROLES) ? names[role] : "?";
}

int cp_model_profile_roles(cp_model* m, double* out, int num_roles) {
    if (!m || !out || num_roles < CP_NUM_ROLES) return fail(CP_ERR_INVALID, "bad argument");
    for (int i = 0; i < CP_NUM_ROLES * 4; ++i) out[i] = m->roles[i];
    return CP_OK;
}

size_t cp_model_workspace_used(const cp_model* m) { return m ? m->arena.peak : 0; }
int cp_model_maxpool_launches(const cp_model* m) { return m ? m->maxpool2_launches : 0; }

size_t cp_model_workspace_bytes(cp_model* m, int B, int H, int W) {
    if (!m) {
        fail(CP_ERR_STATE, "cp_model_workspace_bytes: null model");
        return 0;
    }
    // The launch sequence -- and with it the arena's allocation order -- has forms the caller may select later (cp_model::DryForm).
    // The query runs the dry pass for every combination of them and returns the largest peak: every sequence a real pass can take
    // is one of these, so its peak is at most the one returned here (cp_model_workspace_used reads a real pass's back).
    if (m->ws_cached && m->ws_key[0] == B && m->ws_key[1] == H && m->ws_key[2] == W && m->ws_key[3] == g_dbg && m->finalized)
        return m->ws_cached;   // (cp_model_detect asks on every call: up to 48 dry passes per frame would show in the batch-1 latency)
    using Form = cp_model::DryForm;
    size_t peak = 0;
    const char* const tap_before = m->tap_name;
    m->tap_name = nullptr;
    const int n_ida = m->ups_t.empty() ? 1 : 3;  // models without an IDAUp have one form of it
    const int n_entry = m->convs.count("base.level2.project") ? 2 : 1;  // ... without DLA's level entries one of those (projection, pooled input)
    int rc = CP_OK;
    for (int pool = 0; pool < n_entry; ++pool)
        for (int proj = 0; proj < n_entry; ++proj)
            for (int ida = 0; ida < n_ida; ++ida)
                for (int tap = 0; tap < 2; ++tap)
                    for (int stem = 0; stem < 2 && rc == CP_OK; ++stem) {
                        m->form.stem_level0_fused = stem == 1;
                        m->form.tap_routing = tap == 1;
                        m->form.idaup = ida == 0 ? Form::IDA_ALL : ida == 1 ? Form::IDA_NONE : Form::IDA_BOUNDARY;
                        m->form.project_unfused = proj == 1;
                        m->form.no_pooled_producer = pool == 1;
                        rc = forward_impl(m, nullptr, B, H, W, nullptr, (const float*)1, (const float*)1, (const float*)1, nullptr, 0,
                                          nullptr, 0, true);
                        if (m->arena.peak > peak) peak = m->arena.peak;
                    }
    m->form = Form();
    m->tap_name = tap_before;
    if (rc != CP_OK) return 0;
    m->ws_key[0] = B; m->ws_key[1] = H; m->ws_key[2] = W; m->ws_key[3] = g_dbg;
    m->ws_cached = peak;
    return peak;
}

int cp_model_forward(cp_model* m, cp_stream_t stream, int B, int H, int W, const float* images, const float* pre_img,
                     const float* pre_hm, const float* pre_hm_hp, float* const* head_out, int sigmoid_hm,
                     void* workspace, size_t workspace_bytes) {
    if (!m || !images || !head_out || !workspace) return fail(CP_ERR_INVALID, "null argument");
    if (const int rc = workspace_refused(m, "cp_model_forward", B, H, W, workspace_bytes)) return rc;
    m->tap_name = nullptr;
    drop_kept_in(m, workspace, workspace_bytes);
    return forward_impl(m, (hipStream_t)stream, B, H, W, images, pre_img, pre_hm, pre_hm_hp, head_out, sigmoid_hm,
                        workspace, workspace_bytes, false);
}

int cp_model_features(cp_model* m, cp_stream_t stream, int B, int H, int W, const float* images, const float* pre_img,
                      const float* pre_hm, const float* pre_hm_hp, float* feat_out, void* workspace, size_t workspace_bytes) {
    if (!m || !images || !feat_out || !workspace) return fail(CP_ERR_INVALID, "null argument");
    if (m->gru) return fail(CP_ERR_STATE, "cp_model_features: dlav1 heads read the ConvGRU steps through GroupNorm, not one feature map");
    if (m->hourglass) return fail(CP_ERR_STATE, "cp_model_features: hourglass has two stacks of heads, not one feature map");
    if (const int rc = workspace_refused(m, "cp_model_features", B, H, W, workspace_bytes)) return rc;
    m->tap_name = nullptr;
    drop_kept_in(m, workspace, workspace_bytes);
    m->feat_out = feat_out;
    const int rc = forward_impl(m, (hipStream_t)stream, B, H, W, images, pre_img, pre_hm, pre_hm_hp, nullptr, 0, workspace,
                                workspace_bytes, false);
    m->feat_out = nullptr;
    return rc;
}

// the decode's share of a detect workspace: peaks_kernel up to 32768 output pixels, the tiled peaks above (0: unsupported)
static size_t detect_decode_ws_bytes(int B, int H, int W, int K) {
    const int ho = H / 4, wo = W / 4;
    return ho * wo <= 32768 ? cp_decode_ws_bytes(B, 8, K) : cp_decode_tiled_ws_bytes(B, 8, ho, wo, K);
}

size_t cp_model_detect_workspace_bytes(cp_model* m, int B, int H, int W, int K) {
    const size_t a = cp_model_workspace_bytes(m, B, H, W);
    const size_t d = detect_decode_ws_bytes(B, H, W, K);
    return a && d ? align_up(a, 256) + d : 0;
}

// backbone + heads + sigmoid + decode in one call (what ObjectPoseDetector.process does, object_pose.py:131-165),
// optionally replayed from a captured hipGraph (the ~120 launches of a frame become one graph launch).
// Every head is computed on every output pixel here, although the decode reads the regression heads at the peaks only: those dense maps
// are a by-product.  cp_model_detect_lean below leaves them out (and cp_model_dense_heads computes them on request, at their old cost).
int cp_model_detect(cp_model* m, cp_stream_t stream, int B, int H, int W, const float* images, const float* pre_img,
                    const float* pre_hm, const float* pre_hm_hp, float* const* head_out, int K, int rep_mode,
                    int fit_gaussian, float balance, int legacy_bool_mask, float* det, void* workspace,
                    size_t workspace_bytes, int use_graph) {
    if (!m || !images || !head_out || !det || !workspace) return fail(CP_ERR_INVALID, "null argument");
    if (!m->finalized) return fail(CP_ERR_STATE, "model not finalized");
    const size_t model_ws = align_up(cp_model_workspace_bytes(m, B, H, W), 256);
    if (model_ws == 0) return CP_ERR_INVALID;
    const bool tiled = (H / 4) * (W / 4) > 32768;
    const size_t dec_ws = detect_decode_ws_bytes(B, H, W, K);
    if (dec_ws == 0) return fail(CP_ERR_INVALID, "detect: unsupported decode shape (need K <= 128, K <= H*W/16 <= 2^20, W/4 <= 4096)");
    if (workspace_bytes < model_ws + dec_ws)
        return fail(CP_ERR_INVALID, "cp_model_detect: workspace too small: " + std::to_string(workspace_bytes) +
                                        " bytes given, cp_model_detect_workspace_bytes asks for " + std::to_string(model_ws + dec_ws));
    // decode inputs by head name (opts.py:394-426)
    float* hp[11] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const char* names[11] = {"hm", "hps", "wh", "hps_uncertainty", "scale", "scale_uncertainty", "reg", "hm_hp",
                             "hp_offset", "tracking", "tracking_hp"};
    for (size_t i = 0; i < m->headw.size(); ++i)
        for (int j = 0; j < 11; ++j)
            if (m->headw[i].name == names[j]) hp[j] = head_out[i];
    if (!hp[0] || !hp[1] || !hp[2] || !hp[7]) return fail(CP_ERR_INVALID, "detect needs the hm, hps, wh and hm_hp heads");
    hipStream_t s = (hipStream_t)stream;
    auto enqueue = [&]() -> int {
        m->tap_name = nullptr;
        int rc = forward_impl(m, s, B, H, W, images, pre_img, pre_hm, pre_hm_hp, head_out, 1, workspace, model_ws, false);
        if (rc != CP_OK) return rc;
        rc = timed(m, s, [&](cp_model::ProfRec& r) {
            // algorithmic bytes of the decode: one read of hm + hm_hp, the gathers at the K centres
            // (<= 60 channels) and at the 8K joint peaks (2 channels), the records written
            const double hw = (double)(H / 4) * (W / 4);
            r.variant = CP_VARIANT_NONE;
            r.role = CP_ROLE_DECODE;
            r.flops = 0.0;
            r.bytes = (double)B * (9.0 * hw * 4 + K * 60.0 * 4 + 8.0 * K * 2 * 4 + (double)K * CP_DET_STRIDE * 4);
            r.M = B; r.N = K; r.K = (int)hw; r.kh = 0; r.stride = 0;
        }, [&]() {
            return (tiled ? cp_launch_decode_tiled : cp_launch_decode)(
                s, B, 8, H / 4, W / 4, hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], hp[7], hp[8], hp[9], hp[10], K, rep_mode,
                fit_gaussian, balance, legacy_bool_mask, 0, det, (char*)workspace + model_ws);
        });
        if (rc != CP_OK) return fail(rc, "detect: decode failed (need K <= 128, K <= H*W/16 <= 2^20, W/4 <= 4096)");
        return rc;
    };
    drop_kept_in(m, workspace, workspace_bytes);
    if (!use_graph || m->profile) return enqueue();
    std::vector<uint64_t> key = {(uint64_t)B, (uint64_t)H, (uint64_t)W, (uint64_t)images, (uint64_t)pre_img,
                                 (uint64_t)pre_hm, (uint64_t)pre_hm_hp, (uint64_t)K, (uint64_t)rep_mode,
                                 (uint64_t)fit_gaussian, (uint64_t)legacy_bool_mask, (uint64_t)det, (uint64_t)workspace,
                                 (uint64_t)m->precision, (uint64_t)(balance * 1e6f), (uint64_t)s, (uint64_t)(unsigned)g_dbg};
    for (size_t i = 0; i < m->headw.size(); ++i) key.push_back((uint64_t)head_out[i]);
    return replay_or_capture(m, s, key, enqueue);
}

int cp_model_lean_supported(cp_model* m, int B, int H, int W) {
    if (!m || !m->finalized) return 0;
    if (m->gru || m->resnet || m->precision != CP_PREC_F16X3 || !m->hm_group.ok || !m->reg_group.ok) return 0;
    if (m->lean_key[0] == B && m->lean_key[1] == H && m->lean_key[2] == W && m->lean_key[3] == g_dbg && m->lean_key[4] == m->precision)
        return m->lean_ok ? 1 : 0;
    // the forward pass itself decides (a dry run of it, as for the work-space query)
    cp_model::LeanCall lc;
    std::memset(&lc, 0, sizeof(lc));
    lc.K = 1;
    const char* const tap_before = m->tap_name;
    m->tap_name = nullptr;
    m->lean = &lc;
    m->lean_taken = false;
    const int rc = forward_impl(m, nullptr, B, H, W, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, 0, true);
    m->lean = nullptr;
    m->tap_name = tap_before;
    m->lean_key[0] = B; m->lean_key[1] = H; m->lean_key[2] = W; m->lean_key[3] = g_dbg; m->lean_key[4] = m->precision;
    m->lean_ok = rc == CP_OK && m->lean_taken;
    return m->lean_ok ? 1 : 0;
}

// behind the model's arena: the tiled peaks' candidates, then the slabs of the pixel-list launches
static size_t lean_scratch_bytes(cp_model* m, int B, int H, int W, int K) {
    const size_t cand = cp_decode_cand_bytes(B, 8, H / 4, W / 4, K);
    if (cand == (size_t)-1 || K < 1 || K > 128 || (long long)(H / 4) * (W / 4) < K) return 0;
    // (models whose grouped head launch goes through slabs, the hourglass: room for cp_model_dense_heads' too)
    const size_t dense = lean_finished_maps(m) ? 0 : lean_slab_bytes(m, (size_t)B * (H / 4) * (W / 4));
    return align_up(cand, 256) + lean_slab_bytes(m, (size_t)B * 8 * K) + dense + 256;
}

size_t cp_model_detect_lean_workspace_bytes(cp_model* m, int B, int H, int W, int K) {
    if (!cp_model_lean_supported(m, B, H, W)) return 0;
    const size_t a = cp_model_workspace_bytes(m, B, H, W);
    const size_t d = lean_scratch_bytes(m, B, H, W, K);
    return a && d ? align_up(a, 256) + d : 0;
}

int cp_model_detect_lean(cp_model* m, cp_stream_t stream, int B, int H, int W, const float* images, const float* pre_img,
                         const float* pre_hm, const float* pre_hm_hp, float* const* head_out, float* const* table_out,
                         float* pk_score, int* pk_ind, int K, int rep_mode, int fit_gaussian, float balance,
                         int legacy_bool_mask, float* det, void* workspace, size_t workspace_bytes, int use_graph) {
    if (!m || !images || !head_out || !table_out || !pk_score || !pk_ind || !det || !workspace)
        return fail(CP_ERR_INVALID, "null argument");
    if (!m->finalized) return fail(CP_ERR_STATE, "model not finalized");
    if (!cp_model_lean_supported(m, B, H, W))
        return fail(CP_ERR_STATE, "lean detect: this model / shape / switch setting runs the dense heads (cp_model_lean_supported)");
    const size_t model_ws = align_up(cp_model_workspace_bytes(m, B, H, W), 256);
    const size_t scratch = lean_scratch_bytes(m, B, H, W, K);
    if (model_ws == 0) return CP_ERR_INVALID;
    if (scratch == 0) return fail(CP_ERR_INVALID, "detect: unsupported decode shape (need K <= 128, K <= H*W/16 <= 2^20, W/4 <= 4096)");
    if (workspace_bytes < model_ws + scratch)
        return fail(CP_ERR_INVALID, "cp_model_detect_lean: workspace too small: " + std::to_string(workspace_bytes) +
                                        " bytes given, cp_model_detect_lean_workspace_bytes asks for " + std::to_string(model_ws + scratch));
    for (size_t i = 0; i < m->headw.size(); ++i) {
        const bool map = m->headw[i].name == "hm" || m->headw[i].name == "hm_hp";
        if (map ? !head_out[i] : !table_out[i]) return fail(CP_ERR_INVALID, "lean detect: hm / hm_hp need a map, every other head a table");
    }
    hipStream_t s = (hipStream_t)stream;
    cp_model::LeanCall lc;
    lc.table_out = table_out;
    lc.pk_score = pk_score;
    lc.pk_ind = pk_ind;
    lc.scratch = (char*)workspace + model_ws;
    lc.dense_slabs = lean_finished_maps(m) ? nullptr
                                           : (float*)((char*)lc.scratch + align_up(cp_decode_cand_bytes(B, 8, H / 4, W / 4, K), 256) +
                                                      lean_slab_bytes(m, (size_t)B * 8 * K));
    lc.K = K; lc.rep_mode = rep_mode; lc.fit_gaussian = fit_gaussian; lc.legacy_bool_mask = legacy_bool_mask;
    lc.balance = balance;
    lc.det = det;
    m->kept = cp_model::KeptFeat();
    auto enqueue = [&]() -> int {
        m->tap_name = nullptr;
        m->lean = &lc;
        const int rc = forward_impl(m, s, B, H, W, images, pre_img, pre_hm, pre_hm_hp, head_out, 1, workspace, model_ws, false);
        m->lean = nullptr;
        return rc;
    };
    if (!use_graph || m->profile) return enqueue();
    std::vector<uint64_t> key = {(uint64_t)B, (uint64_t)H, (uint64_t)W, (uint64_t)images, (uint64_t)pre_img,
                                 (uint64_t)pre_hm, (uint64_t)pre_hm_hp, (uint64_t)K, (uint64_t)rep_mode,
                                 (uint64_t)fit_gaussian, (uint64_t)legacy_bool_mask, (uint64_t)det, (uint64_t)workspace,
                                 (uint64_t)m->precision, (uint64_t)(balance * 1e6f), (uint64_t)s, (uint64_t)(unsigned)g_dbg,
                                 (uint64_t)pk_score, (uint64_t)pk_ind, ~(uint64_t)0 /* lean */};
    for (size_t i = 0; i < m->headw.size(); ++i) {
        key.push_back((uint64_t)head_out[i]);
        key.push_back((uint64_t)table_out[i]);
    }
    const int rc = replay_or_capture(m, s, key, enqueue);
    if (rc != CP_OK) return rc;
    // a replay runs no host code: where the feature map lives was noted when the graph was captured
    if (m->kept.ptr) m->graph_kept[key] = m->kept;
    else {
        auto it = m->graph_kept.find(key);
        if (it != m->graph_kept.end()) m->kept = it->second;
    }
    return CP_OK;
}

int cp_model_dense_heads(cp_model* m, cp_stream_t stream, float* const* head_out) {
    if (!m || !head_out) return fail(CP_ERR_INVALID, "null argument");
    if (!m->kept.ptr) return fail(CP_ERR_STATE, "dense heads: no feature map kept (the last call on this model was not a lean detect)");
    for (int i : m->reg_group.idx)
        if (!head_out[i]) return fail(CP_ERR_INVALID, "dense heads: no output for head " + m->headw[i].name);
    return kept_dense_heads(m, (hipStream_t)stream, head_out);
}

size_t cp_model_heads_at_workspace_bytes(cp_model* m, int B, int n) {
    if (!m || !m->reg_group.ok || B < 1 || n < 1) return 0;
    return lean_slab_bytes(m, (size_t)B * n) + 256;
}

int cp_model_heads_at(cp_model* m, cp_stream_t stream, const int* index, int n, float* const* table_out, void* workspace,
                      size_t workspace_bytes) {
    if (!m || !index || !table_out || !workspace || n < 1) return fail(CP_ERR_INVALID, "bad argument");
    if (!m->kept.ptr) return fail(CP_ERR_STATE, "heads at pixels: no feature map kept (the last call on this model was not a lean detect)");
    if (workspace_bytes < cp_model_heads_at_workspace_bytes(m, m->kept.B, n) || ((uintptr_t)workspace & 15u))
        return fail(CP_ERR_INVALID, "workspace too small or not 16-byte aligned");
    return kept_heads_at(m, (hipStream_t)stream, index, n, table_out, (float*)workspace);
}

int cp_model_forward_tap(cp_model* m, cp_stream_t stream, int B, int H, int W, const float* images,
                         const float* pre_img, const float* pre_hm, const float* pre_hm_hp, float* const* head_out,
                         int sigmoid_hm, void* workspace, size_t workspace_bytes, const char* tap_name, float* tap_out,
                         int* tap_dims) {
    if (!m || !images || !head_out || !workspace) return fail(CP_ERR_INVALID, "null argument");
    if (const int rc = workspace_refused(m, "cp_model_forward_tap", B, H, W, workspace_bytes)) return rc;
    drop_kept_in(m, workspace, workspace_bytes);
    m->tap_name = tap_name;
    m->tap_out = tap_out;
    m->tap_dims = tap_dims;
    int rc = forward_impl(m, (hipStream_t)stream, B, H, W, images, pre_img, pre_hm, pre_hm_hp, head_out, sigmoid_hm,
                          workspace, workspace_bytes, false);
    m->tap_name = nullptr;
    return rc;
}

int cp_preprocess(cp_stream_t stream, const unsigned char* image_hwc_bgr, int H, int W, const double* trans6,
                  const float* mean3, const float* std3, float* out_chw, int out_h, int out_w) {
    if (!image_hwc_bgr || !trans6 || !mean3 || !std3 || !out_chw || H < 1 || W < 1 || out_h < 1 || out_w < 1)
        return fail(CP_ERR_INVALID, "bad argument");
    return cp_launch_preprocess(image_hwc_bgr, 1, H, W, trans6, mean3, std3, out_chw, out_h, out_w, (hipStream_t)stream);
}

int cp_preprocess_batch(cp_stream_t stream, const unsigned char* images_bhwc_bgr, int B, int H, int W, const double* trans6,
                        const float* mean3, const float* std3, float* out_bchw, int out_h, int out_w) {
    if (!images_bhwc_bgr || !trans6 || !mean3 || !std3 || !out_bchw || B < 1 || B > 65535 || H < 1 || W < 1 || out_h < 1 || out_w < 1)
        return fail(CP_ERR_INVALID, "bad argument");
    return cp_launch_preprocess(images_bhwc_bgr, B, H, W, trans6, mean3, std3, out_bchw, out_h, out_w, (hipStream_t)stream);
}

int cp_resize_u8(cp_stream_t stream, const unsigned char* image_hwc, int H, int W, int C, unsigned char* out_hwc, int out_h,
                 int out_w) {
    if (!image_hwc || !out_hwc || H < 1 || W < 1 || C < 1 || C > 4 || out_h < 1 || out_w < 1)
        return fail(CP_ERR_INVALID, "bad argument");
    return cp_launch_resize_u8(image_hwc, H, W, C, out_hwc, out_h, out_w, (hipStream_t)stream);
}

int cp_render_gaussians(cp_stream_t stream, const double* recs, int N, float* out, int C, int H, int W, int clear) {
    if (!out || C < 1 || H < 1 || W < 1 || N < 0 || (N > 0 && !recs)) return fail(CP_ERR_INVALID, "bad argument");
    if (clear && hipMemsetAsync(out, 0, (size_t)C * H * W * sizeof(float), (hipStream_t)stream) != hipSuccess)
        return fail(CP_ERR_LAUNCH, "memset failed");
    return cp_launch_render_gaussians(recs, N, out, C, H, W, (hipStream_t)stream);
}

size_t cp_postprocess_workspace_bytes(int B, int K) {
    return B > 0 && K > 0 ? (size_t)B * K * CP_POST_STRIDE * sizeof(double) : 0;
}

int cp_postprocess(cp_stream_t stream, const float* det, int B, int K, const double* meta, double vis_thresh, int nms,
                   float div_scale, double* out, int* count, void* workspace, size_t workspace_bytes) {
    if (!det || !meta || !out || !count || !workspace || B < 1) return fail(CP_ERR_INVALID, "bad argument");
    if (K < 1 || K > 128) return fail(CP_ERR_INVALID, "K must be in [1, 128]");
    if (workspace_bytes < cp_postprocess_workspace_bytes(B, K)) return fail(CP_ERR_INVALID, "workspace too small");
    if (!(div_scale > 0.f)) return fail(CP_ERR_INVALID, "div_scale must be positive");
    return cp_launch_postprocess(det, B, K, meta, vis_thresh, nms, div_scale, out, count, (double*)workspace,
                                 (hipStream_t)stream);
}

size_t cp_pnp_workspace_bytes(int N) { return cp_pnp_ws_bytes(N); }

int cp_pnp_solve(cp_stream_t stream, const float* pts, const float* scale, const double* cam, int N, int npts,
                 double* out, void* workspace, size_t workspace_bytes) {
    if (N == 0) return CP_OK;
    if (!pts || !scale || !cam || !out || !workspace || N < 0) return fail(CP_ERR_INVALID, "null argument");
    if (npts != 8 && npts != 16) return fail(CP_ERR_INVALID, "npts must be 8 or 16");
    if (workspace_bytes < cp_pnp_ws_bytes(N)) return fail(CP_ERR_INVALID, "workspace too small");
    return cp_launch_pnp((hipStream_t)stream, pts, scale, cam, N, npts, out, workspace);
}

// workspace: [pts B*K*16*2 f32][scale B*K*3 f32][cam B*K*4 f64][solver workspace]
size_t cp_pnp_from_post_workspace_bytes(int B, int K) {
    if (B < 1 || K < 1) return 0;
    const size_t n = (size_t)B * K;
    return align_up(n * 32 * 4, 256) + align_up(n * 3 * 4, 256) + align_up(n * 4 * 8, 256) + cp_pnp_ws_bytes((int)n);
}

int cp_pnp_from_post(cp_stream_t stream, const double* post, const int* count, int B, int K, int rep_mode,
                     const double* cam, double* out, void* workspace, size_t workspace_bytes) {
    if (!post || !count || !cam || !out || !workspace || B < 1 || K < 1) return fail(CP_ERR_INVALID, "bad argument");
    if (rep_mode < 0 || rep_mode > 4 || rep_mode == 2)
        return fail(CP_ERR_INVALID, "rep_mode 0, 1, 3 or 4 (2 samples a GMM with numpy's RNG: host only)");
    if (workspace_bytes < cp_pnp_from_post_workspace_bytes(B, K)) return fail(CP_ERR_INVALID, "workspace too small");
    const size_t n = (size_t)B * K;
    const int npts = rep_mode == 1 ? 16 : 8;
    char* w = (char*)workspace;
    float* pts = (float*)w;
    w += align_up(n * 32 * 4, 256);
    float* scale = (float*)w;
    w += align_up(n * 3 * 4, 256);
    double* camn = (double*)w;
    w += align_up(n * 4 * 8, 256);
    int rc = cp_launch_pnp_assemble(post, count, B, K, npts, cam, pts, scale, camn, (hipStream_t)stream);
    if (rc != CP_OK) return fail(rc, "pnp assemble launch failed");
    rc = cp_launch_pnp((hipStream_t)stream, pts, scale, camn, (int)n, npts, out, w);
    return rc == CP_OK ? CP_OK : fail(rc, "pnp launch failed");
}

static_assert(sizeof(cp_track_params) == sizeof(TrackParams), "cp_track_params mirrors TrackParams field by field");

size_t cp_track_state_bytes(int B, int cap) {
    return (B >= 1 && cap >= 1 && cap <= CP_TRACK_CAP) ? cp_track_state_bytes_impl(B, cap) : 0;
}

size_t cp_track_workspace_bytes(int B, int K, int cap) {
    return (B >= 1 && K >= 1 && K <= 128 && cap >= 1 && cap <= CP_TRACK_CAP) ? cp_track_ws_bytes_impl(B, K, cap) : 0;
}

int cp_track_reset(cp_stream_t stream, void* state, int B, int cap) {
    const size_t n = cp_track_state_bytes(B, cap);
    if (!state || n == 0) return fail(CP_ERR_INVALID, "cp_track_reset: bad argument");
    return hipMemsetAsync(state, 0, n, (hipStream_t)stream) == hipSuccess ? CP_OK : fail(CP_ERR_LAUNCH, "memset failed");
}

int cp_track_step(cp_stream_t stream, const cp_track_params* params, const double* vmeta, const double* post, const int* count,
                  const double* det_pnp, int B, void* state, double* render_recs, void* workspace, size_t workspace_bytes) {
    if (!params || !vmeta || !post || !count || !state || !render_recs || !workspace || B < 1)
        return fail(CP_ERR_INVALID, "cp_track_step: null argument");
    TrackParams P;
    std::memcpy(&P, params, sizeof(P));
    if (P.K < 1 || P.K > 128 || P.cap < 1 || P.cap > CP_TRACK_CAP)
        return fail(CP_ERR_INVALID, "cp_track_step: K must be in [1, 128] and cap in [1, CP_TRACK_CAP]");
    if (!P.kalman && !P.scale_pool)
        return fail(CP_ERR_INVALID, "cp_track_step: needs opt.kalman and / or opt.scale_pool (host tracker otherwise)");
    if (P.use_pnp && !det_pnp) return fail(CP_ERR_INVALID, "cp_track_step: use_pnp needs the detections' PnP rows");
    if (P.cat_rule < 0 || P.cat_rule > 2) return fail(CP_ERR_INVALID, "cp_track_step: cat_rule must be 0, 1 or 2");
    if (workspace_bytes < cp_track_workspace_bytes(B, P.K, P.cap)) return fail(CP_ERR_INVALID, "workspace too small");
    const int rc = cp_launch_track_step((hipStream_t)stream, P, vmeta, post, count, P.use_pnp ? det_pnp : nullptr, B, P.K,
                                        state, render_recs, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "cp_track_step: launch failed");
}

static_assert(CP_SEED_STRIDE == SD_PRESENT + 1 && SD_POST + (TR_LOC - TR_POST) == SD_PNP &&
                  SD_PNP + (TR_KF_X - TR_KPS_PNP) == SD_KPS_GT && SD_KPS_GT + 18 == SD_PRESENT,
              "the seed record of include/centerpose_hip.h is the one track_common.h reads");

int cp_track_seed(cp_stream_t stream, const cp_track_params* params, const double* vmeta, const double* seeds,
                  const int* seed_count, const int* gt_render, int B, int S, void* state, double* render_recs) {
    if (!params || !vmeta || !seeds || !seed_count || !state || !render_recs)
        return fail(CP_ERR_INVALID, "cp_track_seed: null argument");
    if (B < 1) return fail(CP_ERR_INVALID, "cp_track_seed: B must be >= 1");
    if (S < 1 || S > CP_TRACK_CAP) return fail(CP_ERR_INVALID, "cp_track_seed: S must be in [1, CP_TRACK_CAP]");
    TrackParams P;
    std::memcpy(&P, params, sizeof(P));
    if (P.cap < 1 || P.cap > CP_TRACK_CAP) return fail(CP_ERR_INVALID, "cp_track_seed: cap must be in [1, CP_TRACK_CAP]");
    const int rc = cp_launch_track_seed((hipStream_t)stream, P, vmeta, seeds, seed_count, gt_render, B, S, state, render_recs);
    return rc == CP_OK ? CP_OK : fail(rc, "cp_track_seed: launch failed");
}

int cp_box_iou(cp_stream_t stream, const double* a, const double* b, int n, double* iou) {
    if (n < 1) return fail(CP_ERR_INVALID, "cp_box_iou: n must be >= 1");
    if (!a || !b || !iou) return fail(CP_ERR_INVALID, "cp_box_iou: null argument");
    return cp_launch_box_iou((hipStream_t)stream, a, b, n, iou);
}

int cp_box_eval(cp_stream_t stream, const double* pred3d, const double* gt3d, const double* pred2d, const double* mo2c,
                const double* proj, const int* single_rotation, int n, int num_symmetry, double* out) {
    if (n < 1) return fail(CP_ERR_INVALID, "cp_box_eval: n must be >= 1");
    if (num_symmetry < 1) return fail(CP_ERR_INVALID, "cp_box_eval: num_symmetry must be >= 1");
    if (!pred3d || !gt3d || !pred2d || !mo2c || !proj || !single_rotation || !out)
        return fail(CP_ERR_INVALID, "cp_box_eval: null argument");
    return cp_launch_box_eval((hipStream_t)stream, pred3d, gt3d, pred2d, mo2c, proj, single_rotation, n, num_symmetry,
                              out);
}

size_t cp_pose_loss_workspace_bytes(const cp_pose_loss_desc* d) { return cp_pose_loss_ws_bytes(d); }

int cp_pose_loss_forward(cp_stream_t stream, const cp_pose_loss_desc* d, float* loss, float* stats, long long* choice,
                         float* terms_out, void* workspace, size_t workspace_bytes) {
    if (const char* e = cp_pose_loss_check(d)) return fail(CP_ERR_INVALID, e);
    if (!loss || !stats || !choice || !workspace) return fail(CP_ERR_INVALID, "pose_loss_forward: null argument");
    if (workspace_bytes < cp_pose_loss_ws_bytes(d)) return fail(CP_ERR_INVALID, "pose_loss_forward: workspace too small");
    const int rc = cp_launch_pose_loss_forward((hipStream_t)stream, d, loss, stats, choice, terms_out, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "pose_loss_forward: kernel launch failed");
}

int cp_pose_loss_backward(cp_stream_t stream, const cp_pose_loss_desc* d, const float* dloss, const float* const* dmaps,
                          float* const* grad, void* workspace, size_t workspace_bytes) {
    if (const char* e = cp_pose_loss_check(d)) return fail(CP_ERR_INVALID, e);
    if (const char* e = cp_pose_loss_check_grads(d, dmaps, grad)) return fail(CP_ERR_INVALID, e);
    if (!dloss || !workspace) return fail(CP_ERR_INVALID, "pose_loss_backward: null argument");
    if (workspace_bytes < cp_pose_loss_ws_bytes(d)) return fail(CP_ERR_INVALID, "pose_loss_backward: workspace too small");
    const int rc = cp_launch_pose_loss_backward((hipStream_t)stream, d, dloss, dmaps, grad, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "pose_loss_backward: kernel launch failed");
}

int cp_linear_assignment(const double* cost, int n_rows, int n_cols, int solver, int* match_out) {
    if (n_rows < 0 || n_cols < 0 || (n_rows > 0 && !match_out) || (n_rows > 0 && n_cols > 0 && !cost) || (solver != 1 && solver != 2))
        return fail(CP_ERR_INVALID, "cp_linear_assignment: bad argument (solver: 1 Munkres, 2 scipy LSAP)");
    for (int i = 0; i < n_rows; ++i)
        for (int j = 0; j < n_cols; ++j)
            if (!std::isfinite(cost[(size_t)i * n_cols + j]))
                return fail(CP_ERR_INVALID, "cp_linear_assignment: non-finite cost at row " + std::to_string(i) + ", column " +
                                                std::to_string(j) + " (forbidden pairs are 1e18, not inf)");
    const size_t ls = (size_t)(n_rows > n_cols ? n_rows : n_cols) + 1;
    auto c = [&](int i, int j) -> double { return cost[(size_t)i * n_cols + j]; };
    try {
        if (solver == 2) {
            std::vector<double> u(ls), v(ls), spc(ls);
            std::vector<int> path(ls), c4r(ls), r4c(ls), rem(ls);
            std::vector<unsigned char> sr(ls), sc(ls);
            const TrkLsapWork W = {u.data(), v.data(), spc.data(), path.data(), c4r.data(), r4c.data(), rem.data(), sr.data(), sc.data()};
            if (!trk_lsap(c, n_rows, n_cols, match_out, W))
                return fail(CP_ERR_INVALID, "cp_linear_assignment: cost matrix is infeasible (costs whose sums overflow float64?)");
        } else {
            std::vector<double> C((size_t)n_rows * n_cols + 1);
            std::vector<unsigned char> marked((size_t)n_rows * n_cols + 1), ru(ls), cu(ls);
            std::vector<int> path(2 * ((size_t)n_rows + n_cols) + 2);
            const TrkMunkresWork W = {C.data(), marked.data(), ru.data(), cu.data(), path.data()};
            if (!trk_munkres(c, n_rows, n_cols, match_out, W))
                return fail(CP_ERR_INVALID, "cp_linear_assignment: Munkres hit its iteration bound (costs whose differences "
                                            "overflow float64?); match_out holds a partial matching");
        }
    } catch (const std::bad_alloc&) {
        return fail(CP_ERR_ALLOC, "cp_linear_assignment: out of host memory");
    }
    return CP_OK;
}

// Sticky per-video overflow counters of the device tracker (list entries dropped because a frame needed more than `cap`
// tracks): dropped_out [B] HOST int32.  Synchronises `stream` (one small copy); call it every few frames, not every frame.
int cp_track_status(cp_stream_t stream, const void* state, int B, int* dropped_out) {
    if (!state || !dropped_out || B < 1) return fail(CP_ERR_INVALID, "cp_track_status: bad argument");
    std::vector<int> hdr(4 + 4 * (size_t)B);
    if (hipMemcpyAsync(hdr.data(), state, hdr.size() * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return fail(CP_ERR_LAUNCH, "cp_track_status: copy failed");
    for (int b = 0; b < B; ++b) dropped_out[b] = hdr[4 + 4 * b + 2];
    return CP_OK;
}

size_t cp_decode_workspace_bytes(int B, int K) { return cp_decode_ws_bytes(B, 8, K); }

int cp_decode(cp_stream_t stream, int B, int H, int W, float* hm, const float* hps, const float* wh,
              const float* hps_uncertainty, const float* scale, const float* scale_uncertainty, const float* reg,
              float* hm_hp, const float* hp_offset, const float* tracking, const float* tracking_hp, int K,
              int rep_mode, int fit_gaussian, float balance, int legacy_bool_mask, int apply_sigmoid, float* det,
              void* workspace, size_t workspace_bytes) {
    if (!hm || !hps || !wh || !hm_hp || !det || !workspace)
        return fail(CP_ERR_INVALID, "hm, hps, wh, hm_hp, det and workspace are required");
    if (B < 1 || rep_mode < 0 || rep_mode > 4) return fail(CP_ERR_INVALID, "bad B / rep_mode");
    if (workspace_bytes < cp_decode_workspace_bytes(B, K)) return fail(CP_ERR_INVALID, "workspace too small");
    int rc = cp_launch_decode((hipStream_t)stream, B, 8, H, W, hm, hps, wh, hps_uncertainty, scale, scale_uncertainty,
                              reg, hm_hp, hp_offset, tracking, tracking_hp, K, rep_mode, fit_gaussian, balance,
                              legacy_bool_mask, apply_sigmoid, det, workspace);
    if (rc != CP_OK) return fail(rc, "decode: unsupported shape (need K <= 128 <= H*W <= 32768, W % 4 == 0) or launch failure");
    return CP_OK;
}

size_t cp_decode_peaks_workspace_bytes(int B, int H, int W, int K) {
    const size_t cand = cp_decode_cand_bytes(B, 8, H, W, K);
    return cand == (size_t)-1 ? 0 : cand + 256;
}

int cp_decode_peaks(cp_stream_t stream, int B, int H, int W, float* hm, float* hm_hp, int K, int apply_sigmoid, float* pk_score,
                    int* pk_ind, void* workspace, size_t workspace_bytes) {
    if (!hm || !hm_hp || !pk_score || !pk_ind || !workspace) return fail(CP_ERR_INVALID, "null argument");
    const size_t need = cp_decode_peaks_workspace_bytes(B, H, W, K);
    if (need == 0) return fail(CP_ERR_INVALID, "unsupported shape (need K <= 128, K <= H*W <= 2^20, W % 4 == 0, W <= 4096)");
    if (workspace_bytes < need || ((uintptr_t)workspace & 15u)) return fail(CP_ERR_INVALID, "workspace too small or not 16-byte aligned");
    const int rc = cp_launch_decode_peaks((hipStream_t)stream, B, 8, H, W, hm, hm_hp, K, apply_sigmoid, pk_score, pk_ind, workspace);
    return rc == CP_OK ? rc : fail(rc, "cp_decode_peaks: launch failed or unsupported shape");
}

int cp_decode_gathered(cp_stream_t stream, int B, int H, int W, const float* hm_hp, const float* hps, const float* wh,
                       const float* hps_uncertainty, const float* scale, const float* scale_uncertainty, const float* reg,
                       const float* hp_offset, const float* tracking, const float* tracking_hp, const float* pk_score,
                       const int* pk_ind, int K, int rep_mode, int fit_gaussian, float balance, int legacy_bool_mask, float* det) {
    if (!hm_hp || !hps || !wh || !pk_score || !pk_ind || !det) return fail(CP_ERR_INVALID, "null argument");
    if (B < 1 || K < 1 || K > 128 || H < 1 || W < 1) return fail(CP_ERR_INVALID, "bad shape");
    const int rc = cp_launch_decode_assoc((hipStream_t)stream, B, 8, H, W, hps, wh, hps_uncertainty, scale, scale_uncertainty, reg,
                                          hm_hp, hp_offset, tracking, tracking_hp, pk_score, pk_ind, K, rep_mode, fit_gaussian,
                                          balance, legacy_bool_mask, 1, det);
    return rc == CP_OK ? rc : fail(rc, "cp_decode_gathered: launch failed");
}

size_t cp_decode_tiled_workspace_bytes(int B, int H, int W, int K) { return cp_decode_tiled_ws_bytes(B, 8, H, W, K); }

int cp_decode_tiled(cp_stream_t stream, int B, int H, int W, float* hm, const float* hps, const float* wh,
                    const float* hps_uncertainty, const float* scale, const float* scale_uncertainty, const float* reg,
                    float* hm_hp, const float* hp_offset, const float* tracking, const float* tracking_hp, int K,
                    int rep_mode, int fit_gaussian, float balance, int legacy_bool_mask, int apply_sigmoid, float* det,
                    void* workspace, size_t workspace_bytes) {
    if (!hm || !hps || !wh || !hm_hp || !det || !workspace)
        return fail(CP_ERR_INVALID, "hm, hps, wh, hm_hp, det and workspace are required");
    if (B < 1 || rep_mode < 0 || rep_mode > 4) return fail(CP_ERR_INVALID, "bad B / rep_mode");
    const size_t need = cp_decode_tiled_workspace_bytes(B, H, W, K);
    if (need == 0)
        return fail(CP_ERR_INVALID, "decode_tiled: unsupported shape (need 1 <= K <= 128, K <= H*W <= 1048576, "
                                    "W % 4 == 0, W <= 4096)");
    if (workspace_bytes < need) return fail(CP_ERR_INVALID, "workspace too small");
    if (((uintptr_t)workspace & 15u) != 0) return fail(CP_ERR_INVALID, "decode_tiled: workspace must be 16-byte aligned");
    int rc = cp_launch_decode_tiled((hipStream_t)stream, B, 8, H, W, hm, hps, wh, hps_uncertainty, scale, scale_uncertainty,
                                    reg, hm_hp, hp_offset, tracking, tracking_hp, K, rep_mode, fit_gaussian, balance,
                                    legacy_bool_mask, apply_sigmoid, det, workspace);
    if (rc != CP_OK) return fail(rc, "decode_tiled: launch failure");
    return CP_OK;
}
size_t cp_pose_targets_workspace_bytes(const cp_pose_targets_desc* d) { return cp_pose_targets_ws_bytes(d); }

int cp_pose_targets(cp_stream_t stream, const cp_pose_targets_desc* d, void* workspace, size_t workspace_bytes) {
    if (const char* e = cp_pose_targets_check(d)) return fail(CP_ERR_INVALID, e);
    if (!workspace) return fail(CP_ERR_INVALID, "pose_targets: null workspace");
    if (workspace_bytes < cp_pose_targets_ws_bytes(d)) return fail(CP_ERR_INVALID, "pose_targets: workspace too small");
    const int rc = cp_launch_pose_targets((hipStream_t)stream, d, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "pose_targets: copy or kernel launch failed");
}

size_t cp_pose_targets_track_workspace_bytes(const cp_pose_targets_track_desc* d) { return cp_pose_targets_track_ws_bytes(d); }

int cp_pose_targets_track(cp_stream_t stream, const cp_pose_targets_track_desc* d, void* workspace, size_t workspace_bytes) {
    if (const char* e = cp_pose_targets_track_check(d)) return fail(CP_ERR_INVALID, e);
    if (!workspace) return fail(CP_ERR_INVALID, "pose_targets_track: null workspace");
    if (workspace_bytes < cp_pose_targets_track_ws_bytes(d))
        return fail(CP_ERR_INVALID, "pose_targets_track: workspace too small");
    const int rc = cp_launch_pose_targets_track((hipStream_t)stream, d, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "pose_targets_track: copy or kernel launch failed");
}

size_t cp_pose_targets_track_det_workspace_bytes(const cp_pose_targets_track_det_desc* d) {
    return cp_pose_targets_track_det_ws_bytes(d);
}

int cp_pose_targets_track_det(cp_stream_t stream, const cp_pose_targets_track_det_desc* d, void* workspace,
                              size_t workspace_bytes) {
    if (const char* e = cp_pose_targets_track_det_check(d)) return fail(CP_ERR_INVALID, e);
    if (!workspace) return fail(CP_ERR_INVALID, "pose_targets_track_det: null workspace");
    if (workspace_bytes < cp_pose_targets_track_det_ws_bytes(d))
        return fail(CP_ERR_INVALID, "pose_targets_track_det: workspace too small");
    const int rc = cp_launch_pose_targets_track_det((hipStream_t)stream, d, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "pose_targets_track_det: copy or kernel launch failed");
}

size_t cp_train_inputs_workspace_bytes(int N, int out_h, int out_w) { return cp_train_inputs_ws_bytes(N, out_h, out_w); }

int cp_train_inputs(cp_stream_t stream, const unsigned char* frames, size_t frames_bytes, const double* records, int N,
                    const float* mean3, const float* std3, float* out, int out_h, int out_w, void* workspace,
                    size_t workspace_bytes) {
    if (const char* e = cp_train_inputs_check(frames, frames_bytes, records, N, mean3, std3, out, out_h, out_w))
        return fail(CP_ERR_INVALID, e);
    if (!workspace) return fail(CP_ERR_INVALID, "train_inputs: null workspace");
    if (workspace_bytes < cp_train_inputs_ws_bytes(N, out_h, out_w))
        return fail(CP_ERR_INVALID, "train_inputs: workspace too small");
    const int rc = cp_launch_train_inputs((hipStream_t)stream, frames, records, N, mean3, std3, out, out_h, out_w, workspace);
    return rc == CP_OK ? CP_OK : fail(rc, "train_inputs: copy or kernel launch failed");
}

}  // extern "C"
