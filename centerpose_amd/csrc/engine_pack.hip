// Parameter folding and packing: cp_model_create / cp_model_set_param collect the checkpoint on the host, cp_model_finalize
// folds BatchNorm and biases and packs every layer's weights into the kernels' operand layouts, once (Packer).
//
// Topology follows the reference modules (paths relative to the reference's src/lib/models/networks):
//   DLA pose_dla_dcn.py:253-322, Tree :211-224, IDAUp :411-417, DeformConv :377-389 (DCN: DCNv2/dcn_v2.py:118-128),
//   ConvGRU convGRU.py:72-94, GroupNorm GN.py:4-9, stacked hourglass large_hourglass.py, PoseResNet resnet_dcn.py.
#include "engine_model.h"

using namespace cp_engine;

namespace {

struct Packer {
    cp_model* m;
    int status = CP_OK;
    std::string missing;

    // a failing HIP runtime call while packing makes cp_model_finalize fail (first error wins)
    bool hip_ok(hipError_t e) {
        if (e != hipSuccess && status == CP_OK) {
            status = CP_ERR_LAUNCH;
            missing = std::string("HIP runtime: ") + hipGetErrorString(e);
        }
        return e == hipSuccess;
    }
    const std::vector<float>* get(const std::string& n, size_t numel) {
        auto it = m->params.find(n);
        if (it == m->params.end() || it->second.size() != numel) {
            if (status == CP_OK) missing = n;
            status = CP_ERR_STATE;
            return nullptr;
        }
        return &it->second;
    }
    float* dev_alloc(size_t nfloat, bool zero = true) {
        void* p = nullptr;
        if (hipMalloc(&p, nfloat * sizeof(float)) != hipSuccess) {
            status = CP_ERR_ALLOC;
            return nullptr;
        }
        if (zero) hip_ok(hipMemset(p, 0, nfloat * sizeof(float)));
        m->device_allocs.push_back(p);
        return (float*)p;
    }
    float* upload(const std::vector<float>& h) {
        float* d = dev_alloc(h.size(), false);
        if (d) hip_ok(hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        return d;
    }
    // fragment-ordered copies of the split-f16 weights (3x3 layers): dcn16p.hip and halo16.hip load their MFMA B operands
    // straight from them
    void frag_copies(ConvW& c) {
        if (c.w16f_hi) return;
        const size_t halfs = (size_t)c.CoutPad * c.Kpad16;
        c.w16f_hi = dev_alloc((halfs + 1) / 2);
        c.w16f_lo = dev_alloc((halfs + 1) / 2);
        if (!c.w16f_hi || !c.w16f_lo) return;
        int rc = cp_launch_frag16_repack(c.w16_hi, c.w16f_hi, c.CoutPad, c.Kpad16, nullptr);
        if (rc == CP_OK) rc = cp_launch_frag16_repack(c.w16_lo, c.w16f_lo, c.CoutPad, c.Kpad16, nullptr);
        hip_ok(hipDeviceSynchronize());
        if (rc != CP_OK) status = rc;
    }
    // Pack several PyTorch-layout weights side by side along Cout (GRU gates) into one GEMM operand.
    ConvW pack(const std::vector<std::string>& wnames, int cout_each, int cin, int kh, int kw, int cin_pad = 0,
               int cout_pad_min = 0) {
        ConvW c;
        c.Cin = cin;
        c.CinP = cin_pad ? cin_pad : cin;
        c.Cout = cout_each * (int)wnames.size();
        c.CoutPad = (int)align_up(c.Cout, cp_conv_tile_n(c.Cout));
        if (c.CoutPad < cout_pad_min) c.CoutPad = cout_pad_min;  // <= 16-wide heads: 32 columns for the f16x3 N tile
        c.KH = kh;
        c.KW = kw;
        c.K = kh * kw * c.CinP;
        c.Kpad = (int)align_up(c.K, 16);
        c.wp = dev_alloc((size_t)c.Kpad * c.CoutPad);
        if (!c.wp) return c;
        const bool want16 = (c.CinP == cin) && (cin % 32 == 0) && c.CoutPad >= 32 && c.CoutPad % 32 == 0 && kh * kw <= 32;
        if (want16) {
            c.Kpad16 = c.K;
            const size_t halfs = (size_t)c.CoutPad * c.Kpad16;
            c.w16_hi = dev_alloc((halfs + 1) / 2);
            c.w16_lo = dev_alloc((halfs + 1) / 2);
            const std::vector<float> ones(c.CoutPad, 1.f);
            c.wfwd = upload(ones);
            c.winv = upload(ones);
            c.scale16 = upload(ones);
            if (!c.w16_hi || !c.w16_lo || !c.wfwd || !c.winv || !c.scale16) return c;
        }
        for (size_t i = 0; i < wnames.size(); ++i) {
            const auto* w = get(wnames[i], (size_t)cout_each * cin * kh * kw);
            if (!w) return c;
            float* tmp = nullptr;
            if (hipMalloc((void**)&tmp, w->size() * sizeof(float)) != hipSuccess) {
                status = CP_ERR_ALLOC;
                return c;
            }
            hip_ok(hipMemcpy(tmp, w->data(), w->size() * sizeof(float), hipMemcpyHostToDevice));
            int rc = cp_launch_pack_weight(tmp, c.wp, cout_each, cin, kh * kw, c.CinP, c.CoutPad, (int)i * cout_each,
                                           nullptr);
            if (rc == CP_OK && c.w16_hi && c.w16_lo) {
                const int coff = (int)i * cout_each;
                rc = cp_launch_weight_scale(tmp, cout_each, cin * kh * kw, c.wfwd + coff, c.winv + coff, nullptr);
                if (rc == CP_OK)
                    rc = cp_launch_pack_weight16(tmp, c.w16_hi, c.w16_lo, cout_each, cin, kh * kw, c.Kpad16, coff, c.wfwd,
                                                 nullptr);
            }
            hip_ok(hipDeviceSynchronize());
            (void)hipFree(tmp);
            if (rc != CP_OK) status = rc;
        }
        if (c.w16_hi && c.w16_lo && ((kh == 3 && kw == 3) || (kh == 1 && kw == 1)) && status == CP_OK) frag_copies(c);
        if (c.scale16 && status == CP_OK) {  // no affine yet: scale16 = winv (set_affine folds a scale in later)
            const int rc = cp_launch_scale16(nullptr, c.winv, c.scale16, c.CoutPad, nullptr);
            hip_ok(hipDeviceSynchronize());
            if (rc != CP_OK) status = rc;
        }
        return c;
    }
    // scale/shift vectors padded to CoutPad (scale pad = 1, shift pad = 0)
    void set_affine(ConvW& c, const std::vector<float>* scale, const std::vector<float>& shift) {
        std::vector<float> sh(c.CoutPad, 0.f);
        for (size_t i = 0; i < shift.size(); ++i) sh[i] = shift[i];
        c.shift = upload(sh);
        if (scale) {
            std::vector<float> sc(c.CoutPad, 1.f);
            for (size_t i = 0; i < scale->size(); ++i) sc[i] = (*scale)[i];
            c.scale = upload(sc);
            if (c.scale && c.scale16) {
                const int rc = cp_launch_scale16(c.scale, c.winv, c.scale16, c.CoutPad, nullptr);
                hip_ok(hipDeviceSynchronize());
                if (rc != CP_OK) status = rc;
            }
        }
    }
    // eval-mode BatchNorm folded to y = x*scale + shift; optional conv bias folded in as well
    bool bn_fold(const std::string& bn, int c, const std::vector<float>* conv_bias, std::vector<float>& scale,
                 std::vector<float>& shift) {
        const auto* g = get(bn + ".weight", c);
        const auto* b = get(bn + ".bias", c);
        const auto* mu = get(bn + ".running_mean", c);
        const auto* var = get(bn + ".running_var", c);
        if (!g || !b || !mu || !var) return false;
        scale.resize(c);
        shift.resize(c);
        for (int i = 0; i < c; ++i) {
            const double s = (double)(*g)[i] / std::sqrt((double)(*var)[i] + 1e-5);
            double t = (double)(*b)[i] - (double)(*mu)[i] * s;
            if (conv_bias) t += (double)(*conv_bias)[i] * s;
            scale[i] = (float)s;
            shift[i] = (float)t;
        }
        return true;
    }
    void conv_bn(const std::string& key, const std::string& conv, const std::string& bn, int cout, int cin, int k,
                 int cin_pad = 0) {
        ConvW c = pack({conv + ".weight"}, cout, cin, k, k, cin_pad);
        std::vector<float> sc, sh;
        if (bn_fold(bn, cout, nullptr, sc, sh)) set_affine(c, &sc, sh);
        m->convs[key] = c;
    }
    void block(const std::string& p, int cin, int cout) {
        conv_bn(p + ".conv1", p + ".conv1", p + ".bn1", cout, cin, 3);
        conv_bn(p + ".conv2", p + ".conv2", p + ".bn2", cout, cout, 3);
    }
    void tree(const std::string& p, int levels, int cin, int cout, bool level_root, int root_dim = 0) {
        if (root_dim == 0) root_dim = 2 * cout;
        if (level_root) root_dim += cin;
        if (levels == 1) {
            block(p + ".tree1", cin, cout);
            block(p + ".tree2", cout, cout);
            conv_bn(p + ".root", p + ".root.conv", p + ".root.bn", cout, root_dim, 1);
            if (cin != cout) conv_bn(p + ".project", p + ".project.0", p + ".project.1", cout, cin, 1);
        } else {
            tree(p + ".tree1", levels - 1, cin, cout, false, 0);
            tree(p + ".tree2", levels - 1, cout, cout, false, root_dim + cout);
            // the outer project of a 2-level tree never influences the output (Tree.forward :214-217)
        }
    }
    // DCN (dcn_v2.py: weight, bias, conv_offset_mask) + BatchNorm `bn`, stored under `key`; the DCN bias folds into the
    // BatchNorm's shift
    void deform(const std::string& key, const std::string& dcn, const std::string& bn, int chi, int cho) {
        DeformW d;
        d.offset = pack({dcn + ".conv_offset_mask.weight"}, 27, chi, 3, 3);
        if (const auto* b = get(dcn + ".conv_offset_mask.bias", 27)) set_affine(d.offset, nullptr, *b);
        d.main = pack({dcn + ".weight"}, cho, chi, 3, 3);
        const auto* bias = get(dcn + ".bias", cho);
        std::vector<float> sc, sh;
        if (bias && bn_fold(bn, cho, bias, sc, sh)) set_affine(d.main, &sc, sh);
        m->deforms[key] = d;
    }
    // DLA's DeformConv (pose_dla_dcn.py:377-389): DCN at `.conv`, BatchNorm at `.actf.0`
    void deform(const std::string& p, int chi, int cho) { deform(p, p + ".conv", p + ".actf.0", chi, cho); }
    void ida(const std::string& p, int o, const std::vector<int>& channels, const std::vector<int>& up_f) {
        for (size_t i = 1; i < channels.size(); ++i) {
            const std::string k = std::to_string(i);
            deform(p + ".proj_" + k, channels[i], o);
            deform(p + ".node_" + k, o, o);
            const int f = up_f[i];
            if (const auto* w = get(p + ".up_" + k + ".weight", (size_t)o * 4 * f * f)) {
                m->ups[p + ".up_" + k] = upload(*w);
                // ... and as [tap][channel] for the DCN epilogue that adds the up-sampled tensor (dcn16t.hip, ConvParams::up_wt)
                const int kk = 4 * f * f;
                std::vector<float> wt((size_t)o * kk);
                for (int c = 0; c < o; ++c)
                    for (int t = 0; t < kk; ++t) wt[(size_t)t * o + c] = (*w)[(size_t)c * kk + t];
                m->ups_t[p + ".up_" + k] = upload(wt);
            }
        }
    }
    // ---- stacked hourglass (large_hourglass.py) ----
    void hg_residual(const std::string& p, int cin, int cout, int stride) {
        conv_bn(p + ".conv1", p + ".conv1", p + ".bn1", cout, cin, 3);
        conv_bn(p + ".conv2", p + ".conv2", p + ".bn2", cout, cout, 3);
        if (stride != 1 || cin != cout) conv_bn(p + ".skip", p + ".skip.0", p + ".skip.1", cout, cin, 1);
    }
    void hg_kp(const std::string& p, int n, const int* dims, const int* mods) {
        const int cur = dims[0], nxt = dims[1], cm = mods[0], nm = mods[1];
        for (int i = 0; i < cm; ++i) hg_residual(p + ".up1." + std::to_string(i), cur, cur, 1);
        for (int i = 0; i < cm; ++i) hg_residual(p + ".low1." + std::to_string(i), i == 0 ? cur : nxt, nxt, i == 0 ? 2 : 1);
        if (n > 1) hg_kp(p + ".low2", n - 1, dims + 1, mods + 1);
        else
            for (int i = 0; i < nm; ++i) hg_residual(p + ".low2." + std::to_string(i), nxt, nxt, 1);
        for (int i = 0; i < cm; ++i) hg_residual(p + ".low3." + std::to_string(i), nxt, i < cm - 1 ? nxt : cur, 1);
    }
    void run_hourglass() {
        static const int dims[6] = {256, 256, 384, 384, 384, 512}, mods[6] = {2, 2, 2, 2, 2, 4};
        conv_bn("pre.0", "pre.0.conv", "pre.0.bn", 128, 3, 7, 4);
        hg_residual("pre.1", 128, 256, 2);
        for (int k = 0; k < 2; ++k) {
            const std::string ks = std::to_string(k);
            hg_kp("kps." + ks, 5, dims, mods);
            conv_bn("cnvs." + ks, "cnvs." + ks + ".conv", "cnvs." + ks + ".bn", 256, 256, 3);
        }
        hg_residual("inters.0", 256, 256, 1);
        conv_bn("inters_.0", "inters_.0.0", "inters_.0.1", 256, 256, 1);
        conv_bn("cnvs_.0", "cnvs_.0.0", "cnvs_.0.1", 256, 256, 1);
        // heads of the LAST stack only: the detector takes model(x)[-1] (object_pose.py:135); the first stack's head
        // tensors do not feed anything downstream
        for (auto& h : m->heads) {
            HeadW hw;
            hw.name = h.first;
            hw.classes = h.second;
            const std::string b = h.first + ".1";
            hw.c0 = pack({b + ".0.conv.weight"}, 256, 256, 3, 3);
            if (const auto* bias = get(b + ".0.conv.bias", 256)) set_affine(hw.c0, nullptr, *bias);
            hw.c1 = pack({b + ".1.weight"}, h.second, 256, 1, 1);
            if (const auto* bias = get(b + ".1.bias", h.second)) set_affine(hw.c1, nullptr, *bias);
            if (h.second <= 32 && hw.c0.w16_hi) {
                if (const auto* w1 = get(b + ".1.weight", (size_t)h.second * 256)) {
                    float* tmp = upload(*w1);
                    hw.w2_hi = dev_alloc((size_t)256 * 32 / 2);
                    hw.w2_lo = dev_alloc((size_t)256 * 32 / 2);
                    hw.w2_inv = dev_alloc(64);
                    if (tmp && hw.w2_hi && hw.w2_lo && hw.w2_inv) {
                        const int rc = cp_launch_pack_head_w2(tmp, hw.w2_hi, hw.w2_lo, hw.w2_inv, h.second, 256, nullptr);
                        hip_ok(hipDeviceSynchronize());
                        if (rc != CP_OK) status = rc;
                    }
                }
            }
            m->headw.push_back(hw);
        }
        group_heads();
    }

    // ---- PoseResNet with DCN up-sampling (resnet_dcn.py) ----
    void run_resnet() {
        bool bott = false;
        int blocks[4] = {0, 0, 0, 0};
        if (!resnet_spec(m->resnet, &bott, blocks)) {
            status = CP_ERR_STATE;
            missing = "resnet depth";
            return;
        }
        conv_bn("conv1", "conv1", "bn1", 64, 3, 7, 4);
        int inp = 64;
        const int exp = bott ? 4 : 1;
        for (int l = 0; l < 4; ++l) {
            const int planes = 64 << l, stride = l ? 2 : 1;
            for (int b = 0; b < blocks[l]; ++b) {
                const std::string p = "layer" + std::to_string(l + 1) + "." + std::to_string(b);
                if (bott) {
                    conv_bn(p + ".conv1", p + ".conv1", p + ".bn1", planes, inp, 1);
                    conv_bn(p + ".conv2", p + ".conv2", p + ".bn2", planes, planes, 3);
                    conv_bn(p + ".conv3", p + ".conv3", p + ".bn3", planes * exp, planes, 1);
                } else {
                    conv_bn(p + ".conv1", p + ".conv1", p + ".bn1", planes, inp, 3);
                    conv_bn(p + ".conv2", p + ".conv2", p + ".bn2", planes, planes, 3);
                }
                if (b == 0 && (stride != 1 || inp != planes * exp))
                    conv_bn(p + ".downsample", p + ".downsample.0", p + ".downsample.1", planes * exp, inp, 1);
                inp = planes * exp;
            }
        }
        static const int filters[3] = {256, 128, 64};
        for (int i = 0; i < 3; ++i) {
            const int c = filters[i];
            const std::string fc = "deconv_layers." + std::to_string(6 * i);
            deform(fc, fc, "deconv_layers." + std::to_string(6 * i + 1), inp, c);
            deconv_bn("deconv_layers." + std::to_string(6 * i + 3), "deconv_layers." + std::to_string(6 * i + 4), c, c);
            inp = c;
        }
        const int hc = m->head_conv;
        for (auto& h : m->heads) {
            HeadW hw;
            hw.name = h.first;
            hw.classes = h.second;
            hw.c0 = pack({h.first + ".0.weight"}, hc, 64, 3, 3);
            if (const auto* b = get(h.first + ".0.bias", hc)) set_affine(hw.c0, nullptr, *b);
            hw.c1 = pack({h.first + ".2.weight"}, h.second, hc, 1, 1);
            if (const auto* b = get(h.first + ".2.bias", h.second)) set_affine(hw.c1, nullptr, *b);
            m->headw.push_back(hw);
        }
    }
    // ConvTranspose2d(cin, cout, 4, 2, 1, bias=False) + BatchNorm2d: the four sub-pixel kernels in both precisions
    void deconv_bn(const std::string& up, const std::string& bn, int cin, int cout) {
        DeconvW d;
        d.Cin = cin;
        d.Cout = cout;
        const auto* w = get(up + ".weight", (size_t)cin * cout * 16);
        std::vector<float> sc, sh;
        if (!w || !bn_fold(bn, cout, nullptr, sc, sh)) return;
        const int cpad = cp_deconv_cout_pad(cout);
        const size_t n = (size_t)4 * cpad * 4 * cin;
        d.wf = dev_alloc(n, false);
        d.hi = dev_alloc((n + 1) / 2, false);
        d.lo = dev_alloc((n + 1) / 2, false);
        d.scale16 = dev_alloc(cpad);
        sc.resize(cpad, 1.f);
        sh.resize(cpad, 0.f);
        d.scale = upload(sc);
        d.shift = upload(sh);
        if (!d.wf || !d.hi || !d.lo || !d.scale16 || !d.scale || !d.shift) return;
        // the raw PyTorch-layout weight and the 2^-e rows are only needed while packing: freed right after
        float *tmp = nullptr, *inv = nullptr;
        if (!hip_ok(hipMalloc((void**)&tmp, w->size() * sizeof(float))) || !hip_ok(hipMalloc((void**)&inv, cpad * sizeof(float)))) {
            (void)hipFree(tmp);
            return;
        }
        int rc = hipMemcpy(tmp, w->data(), w->size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess ? CP_OK : CP_ERR_LAUNCH;
        if (rc == CP_OK) rc = cp_launch_pack_deconv(tmp, d.wf, d.hi, d.lo, inv, cin, cout, nullptr);
        if (rc == CP_OK) rc = cp_launch_scale16(d.scale, inv, d.scale16, cpad, nullptr);
        hip_ok(hipDeviceSynchronize());
        (void)hipFree(tmp);
        (void)hipFree(inv);
        if (rc != CP_OK && status == CP_OK) status = rc;
        m->deconvs[up] = d;
    }

    // concatenate the fused heads' operands for a grouped launch (all heads must be fusable and of one shape): the heads `idx` of
    // m->headw in that order.  `rows`: also the [co][k] copies of the 3x3 weights, which the pixel-list kernel reads.
    void group_heads(cp_model::HeadGroup& g, const std::vector<int>& idx, bool rows) {
        const size_t n = idx.size();
        if (n < 2 || n > CP_MAX_HEAD_GROUP || status != CP_OK) return;
        const ConvW& c = m->headw[idx[0]].c0;
        for (int i : idx) {
            const HeadW& h = m->headw[i];
            if (!h.w2_hi || !h.w2_lo || !h.w2_inv || !h.c0.w16f_hi || !h.c0.w16f_lo || !h.c0.scale16 || !h.c0.shift ||
                h.c0.Cin != c.Cin || h.c0.CoutPad != c.CoutPad || h.c0.Cout != c.CoutPad || h.c0.Kpad16 != c.Kpad16 ||
                h.c0.KH != 3 || h.c0.KW != 3 || c.CoutPad % 128 != 0 || (rows && (!h.c0.w16_hi || !h.c0.w16_lo)))
                return;
        }
        const size_t wbytes = (size_t)c.CoutPad * c.Kpad16 * 2, w2bytes = (size_t)c.CoutPad * 32 * 2;
        g.w16f_hi = dev_alloc(n * wbytes / 4, false);
        g.w16f_lo = dev_alloc(n * wbytes / 4, false);
        if (rows) {
            g.w16_hi = dev_alloc(n * wbytes / 4, false);
            g.w16_lo = dev_alloc(n * wbytes / 4, false);
        }
        g.w2_hi = dev_alloc(n * w2bytes / 4, false);
        g.w2_lo = dev_alloc(n * w2bytes / 4, false);
        g.scale16 = dev_alloc(n * c.CoutPad, false);
        g.shift = dev_alloc(n * c.CoutPad, false);
        g.w2_inv = dev_alloc(n * 64, false);
        if (!g.w16f_hi || !g.w16f_lo || !g.w2_hi || !g.w2_lo || !g.scale16 || !g.shift || !g.w2_inv || (rows && (!g.w16_hi || !g.w16_lo)))
            return;
        for (size_t i = 0; i < n; ++i) {
            const HeadW& h = m->headw[idx[i]];
            const auto d2d = hipMemcpyDeviceToDevice;
            hip_ok(hipMemcpy((char*)g.w16f_hi + i * wbytes, h.c0.w16f_hi, wbytes, d2d));
            hip_ok(hipMemcpy((char*)g.w16f_lo + i * wbytes, h.c0.w16f_lo, wbytes, d2d));
            if (rows) {
                hip_ok(hipMemcpy((char*)g.w16_hi + i * wbytes, h.c0.w16_hi, wbytes, d2d));
                hip_ok(hipMemcpy((char*)g.w16_lo + i * wbytes, h.c0.w16_lo, wbytes, d2d));
            }
            hip_ok(hipMemcpy((char*)g.w2_hi + i * w2bytes, h.w2_hi, w2bytes, d2d));
            hip_ok(hipMemcpy((char*)g.w2_lo + i * w2bytes, h.w2_lo, w2bytes, d2d));
            hip_ok(hipMemcpy(g.scale16 + i * c.CoutPad, h.c0.scale16, (size_t)c.CoutPad * 4, d2d));
            hip_ok(hipMemcpy(g.shift + i * c.CoutPad, h.c0.shift, (size_t)c.CoutPad * 4, d2d));
            hip_ok(hipMemcpy(g.w2_inv + i * 64, h.w2_inv, 64 * 4, d2d));
        }
        g.idx = idx;
        g.Cin = c.Cin;
        g.hid = c.CoutPad;
        g.Kpad16 = c.Kpad16;
        g.ok = status == CP_OK;
    }
    // head_group: every head (cp_model_forward, cp_model_detect).  For cp_model_detect_lean the heads in two groups: the heat-maps
    // the decode reads everywhere (hm, hm_hp), and the regression heads it reads at the peaks only -- the centre-indexed ones first,
    // hp_offset (read at the joint peaks) last.
    void group_heads() {
        std::vector<int> all, maps, reg;
        int hp_off = -1;
        for (int i = 0; i < (int)m->headw.size(); ++i) {
            const std::string& n = m->headw[i].name;
            all.push_back(i);
            if (n == "hm" || n == "hm_hp") maps.push_back(i);
            else if (n == "hp_offset") hp_off = i;
            else reg.push_back(i);
        }
        group_heads(m->head_group, all, false);
        if (!m->head_group.ok || maps.size() != 2 || reg.size() < 2) return;
        m->lean_ncentre = (int)reg.size();
        if (hp_off >= 0) reg.push_back(hp_off);
        group_heads(m->hm_group, maps, false);
        group_heads(m->reg_group, reg, true);
    }

    // weight fragments for the direct low-channel kernels (f16x3 mode); the folded BatchNorm comes from the ConvW
    void lowc(const std::string& name, const std::string& wname, int kind, int cout, int cin, int k, const std::string& affine = "") {
        const auto* w = get(wname + ".weight", (size_t)cout * cin * k * k);
        if (!w) return;
        float* tmp = upload(*w);
        const size_t halfs = cp_lowc_weight_halfs(kind);
        void* hi = dev_alloc(halfs / 2);
        void* lo = dev_alloc(halfs / 2);
        float* fwd = dev_alloc(cout);
        float* inv = dev_alloc(cout);
        LowcW lw;
        lw.hi = hi;
        lw.lo = lo;
        lw.scale16 = dev_alloc(cout);
        if (!tmp || !hi || !lo || !fwd || !inv || !lw.scale16) return;
        int rc = cp_launch_weight_scale(tmp, cout, cin * k * k, fwd, inv, nullptr);
        if (rc == CP_OK) rc = cp_launch_pack_lowc(kind, tmp, hi, lo, fwd, cin, nullptr);
        // the folded BatchNorm of the same layer lives in the ConvW packed under the same name (conv_bn ran first)
        auto it = m->convs.find(affine.empty() ? name : affine);
        if (rc == CP_OK) rc = cp_launch_scale16(it != m->convs.end() ? it->second.scale : nullptr, inv, lw.scale16, cout, nullptr);
        hip_ok(hipDeviceSynchronize());
        if (rc != CP_OK) status = rc;
        m->lowc[name] = lw;
    }
    void run() {
        conv_bn("base.base_layer", "base.base_layer.0", "base.base_layer.1", 16, 3, 7, 4);
        // previous-frame stems: each exists iff its own flag was set when the checkpoint was made
        // (pose_dla_dcn.py:253-271), i.e. iff its weights were supplied
        const bool has_pre_img = m->params.count("base.pre_img_layer.0.weight") != 0;
        const bool has_pre_hm = m->params.count("base.pre_hm_layer.0.weight") != 0;
        const bool has_pre_hm_hp = m->params.count("base.pre_hm_hp_layer.0.weight") != 0;
        if (has_pre_img) conv_bn("base.pre_img_layer", "base.pre_img_layer.0", "base.pre_img_layer.1", 16, 3, 7, 4);
        if (has_pre_hm) conv_bn("base.pre_hm_layer", "base.pre_hm_layer.0", "base.pre_hm_layer.1", 16, 1, 7, 4);
        if (has_pre_hm_hp) conv_bn("base.pre_hm_hp_layer", "base.pre_hm_hp_layer.0", "base.pre_hm_hp_layer.1", 16, 8, 7, 8);
        conv_bn("base.level0", "base.level0.0", "base.level0.1", 16, 16, 3);
        conv_bn("base.level1", "base.level1.0", "base.level1.1", 32, 16, 3);
        // f16x3 fragments of the same layers (after conv_bn: they take the folded BatchNorm from the ConvW)
        lowc("base.base_layer", "base.base_layer.0", 0, 16, 3, 7);
        lowc("base.level0", "base.level0.0", 1, 16, 16, 3);
        {   // fused stem + level0 (lowc2_kernel): level0's weights in kernel-row order, and the bound that replaces the measured
            // |max| of the tensor between the two layers: |relu(bn(conv(x)))_c| <= |s_c| sum|w_c| max|x| + |t_c|
            lowc("base.level0.rows", "base.level0.0", 4, 16, 16, 3, "base.level0");
            const auto* w = get("base.base_layer.0.weight", (size_t)16 * 3 * 49);
            std::vector<float> sc, sh;
            if (w && bn_fold("base.base_layer.1", 16, nullptr, sc, sh)) {
                double bl = 0, bs = 0;
                for (int c = 0; c < 16; ++c) {
                    double l1 = 0;
                    for (int i = 0; i < 147; ++i) l1 += std::fabs((double)(*w)[(size_t)c * 147 + i]);
                    bl = std::max(bl, std::fabs((double)sc[c]) * l1);
                    bs = std::max(bs, std::fabs((double)sh[c]));
                }
                m->stem_bound_l = (float)(bl * 1.0001);
                m->stem_bound_s = (float)(bs * 1.0001);
            }
        }
        lowc("base.level1", "base.level1.0", 2, 32, 16, 3);
        lowc("base.level1.rows", "base.level1.0", 5, 32, 16, 3, "base.level1");   // the row-streaming level1 kernel's fragments
        if (has_pre_img) lowc("base.pre_img_layer", "base.pre_img_layer.0", 0, 16, 3, 7);
        if (has_pre_hm) lowc("base.pre_hm_layer", "base.pre_hm_layer.0", 0, 16, 1, 7);
        if (has_pre_hm_hp) lowc("base.pre_hm_hp_layer", "base.pre_hm_hp_layer.0", 3, 16, 8, 7);
        tree("base.level2", 1, 32, 64, false);
        tree("base.level3", 2, 64, 128, true);
        tree("base.level4", 2, 128, 256, true);
        tree("base.level5", 1, 256, 512, true);
        ida("dla_up.ida_0", 256, {256, 512}, {1, 2});
        ida("dla_up.ida_1", 128, {128, 256, 256}, {1, 2, 2});
        ida("dla_up.ida_2", 64, {64, 128, 128, 128}, {1, 2, 2, 2});
        ida("ida_up", 64, {64, 128, 256}, {1, 2, 4});
        if (m->gru) {
            const std::string c = "convGRU.cell0.";
            m->gru_x = pack({c + "Wir.weight", c + "Wiz.weight", c + "Win.weight"}, 64, 64, 3, 3);
            std::vector<float> b;
            for (const char* g : {"Wir", "Wiz", "Win"}) {
                const auto* v = get(c + g + ".bias", 64);
                if (v) b.insert(b.end(), v->begin(), v->end());
            }
            if (b.size() == 192) set_affine(m->gru_x, nullptr, b);
            m->gru_h = pack({c + "Whr.weight", c + "Whz.weight", c + "Whn.weight"}, 64, 64, 3, 3);
            {   // the same weights in the fused-gate order: N tile t (96 wide) = [r | z | n] of channels 32t .. 32t+31
                const size_t halfs = (size_t)192 * 576;
                m->gru_h16_hi = dev_alloc(halfs / 2);
                m->gru_h16_lo = dev_alloc(halfs / 2);
                m->gru_h16_fwd = dev_alloc(192);
                m->gru_h16_inv = dev_alloc(192);
                const char* gates[3] = {"Whr", "Whz", "Whn"};
                for (int g = 0; g < 3 && m->gru_h16_hi && m->gru_h16_lo && m->gru_h16_fwd && m->gru_h16_inv; ++g) {
                    const auto* w = get(c + gates[g] + ".weight", (size_t)64 * 64 * 9);
                    if (!w) break;
                    float* tmp = upload(*w);
                    if (!tmp) break;
                    for (int t = 0; t < 2; ++t) {
                        const int row = t * 96 + g * 32;
                        int rc = cp_launch_weight_scale(tmp + (size_t)32 * t * 64 * 9, 32, 64 * 9, m->gru_h16_fwd + row,
                                                        m->gru_h16_inv + row, nullptr);
                        if (rc == CP_OK)
                            rc = cp_launch_pack_weight16(tmp + (size_t)32 * t * 64 * 9, m->gru_h16_hi, m->gru_h16_lo, 32, 64, 9,
                                                         576, row, m->gru_h16_fwd, nullptr);
                        if (rc != CP_OK) status = rc;
                    }
                    hip_ok(hipDeviceSynchronize());
                }
                if (m->gru_h16_hi && m->gru_h16_lo && status == CP_OK) {
                    m->gru_h16f_hi = dev_alloc(halfs / 2);
                    m->gru_h16f_lo = dev_alloc(halfs / 2);
                    if (m->gru_h16f_hi && m->gru_h16f_lo) {
                        int rc = cp_launch_frag16_repack(m->gru_h16_hi, m->gru_h16f_hi, 192, 576, nullptr);
                        if (rc == CP_OK) rc = cp_launch_frag16_repack(m->gru_h16_lo, m->gru_h16f_lo, 192, 576, nullptr);
                        hip_ok(hipDeviceSynchronize());
                        if (rc != CP_OK) status = rc;
                    }
                }
            }
        }
        const int hc = m->head_conv;
        for (auto& h : m->heads) {
            HeadW hw;
            hw.name = h.first;
            hw.classes = h.second;
            const std::string last = h.first + (m->gru ? ".3" : ".2");
            hw.c0 = pack({h.first + ".0.weight"}, hc, 64, 3, 3);
            if (const auto* b = get(h.first + ".0.bias", hc)) set_affine(hw.c0, nullptr, *b);
            hw.c1 = pack({last + ".weight"}, h.second, hc, 1, 1, 0, m->gru ? 32 : 0);
            if (const auto* b = get(last + ".bias", h.second)) set_affine(hw.c1, nullptr, *b);
            if (!m->gru && hc % 128 == 0 && h.second <= 32 && hw.c0.w16_hi) {
                // conv3x3 -> ReLU -> conv1x1 head: keep the 1x1 weights as MFMA fragments for the fused kernel too
                if (const auto* w1 = get(last + ".weight", (size_t)h.second * hc)) {
                    float* tmp = upload(*w1);
                    hw.w2_hi = dev_alloc((size_t)hc * 32 / 2);
                    hw.w2_lo = dev_alloc((size_t)hc * 32 / 2);
                    hw.w2_inv = dev_alloc(64);
                    if (tmp && hw.w2_hi && hw.w2_lo && hw.w2_inv) {
                        const int rc = cp_launch_pack_head_w2(tmp, hw.w2_hi, hw.w2_lo, hw.w2_inv, h.second, hc, nullptr);
                        hip_ok(hipDeviceSynchronize());
                        if (rc != CP_OK) status = rc;
                    }
                }
            }
            if (m->gru) {
                const auto* g = get(h.first + ".1.weight", hc);
                const auto* be = get(h.first + ".1.bias", hc);
                if (g && be) {
                    hw.gn_gamma = upload(*g);
                    hw.gn_beta = upload(*be);
                }
            }
            m->headw.push_back(hw);
        }
        if (!m->gru) group_heads();
    }
};

}  // namespace

extern "C" {

int cp_model_create(const char* arch, int tracking_task, int num_heads, const char* const* head_names,
                    const int* head_classes, int head_conv, cp_model** out) {
    if (!arch || !out || num_heads < 1 || !head_names || !head_classes) return fail(CP_ERR_INVALID, "null argument");
    std::string a(arch);
    int resnet = 0;
    for (int d : {18, 34, 50, 101, 152})
        if (a == "resdcn_" + std::to_string(d)) resnet = d;
    if (a != "dla_34" && a != "dlav1_34" && a != "hourglass" && !resnet)
        return fail(CP_ERR_INVALID, "arch must be dla_34, dlav1_34, hourglass or resdcn_18|34|50|101|152");
    if (a == "hourglass" && tracking_task)
        return fail(CP_ERR_INVALID, "the hourglass takes a single frame (large_hourglass.py:266)");
    if (resnet && tracking_task)
        return fail(CP_ERR_INVALID, a + " takes a single frame (resnet_dcn.py: PoseResNet.forward)");
    if (head_conv <= 0 || head_conv % 32 != 0) return fail(CP_ERR_INVALID, "head_conv must be a positive multiple of 32");
    cp_model* m = new cp_model();
    m->arch = a;
    m->gru = (a == "dlav1_34");
    m->hourglass = (a == "hourglass");
    m->resnet = resnet;
    m->tracking = tracking_task != 0;
    m->head_conv = head_conv;
    for (int i = 0; i < num_heads; ++i) m->heads.push_back({head_names[i], head_classes[i]});
    if (m->gru) {
        // ConvGRU models route each head to a fixed step (pose_dla_dcn.py:545-563); the reference leaves any other head
        // out of its output dict (the detector then fails with a KeyError).  Refuse it here instead of returning an
        // unwritten tensor.
        static const char* pose[] = {"hm", "wh", "reg", "hm_hp", "hp_offset", "hps", "scale"};
        static const char* track[] = {"tracking", "tracking_hp", "hps_uncertainty", "scale_uncertainty"};
        for (auto& h : m->heads) {
            bool ok = false;
            for (const char* n : pose) ok = ok || h.first == n;
            if (m->tracking)
                for (const char* n : track) ok = ok || h.first == n;
            if (!ok) {
                const std::string msg = "dlav1_34: head '" + h.first + "' has no ConvGRU step in the reference routing (" +
                                        (m->tracking ? "tracking" : "non-tracking") + " table, pose_dla_dcn.py:545-563)";
                delete m;
                return fail(CP_ERR_INVALID, msg);
            }
        }
    }
    *out = m;
    return CP_OK;
}

int cp_model_set_param(cp_model* m, const char* name, const float* host_data, int64_t numel) {
    if (!m || !name || !host_data || numel < 0) return fail(CP_ERR_INVALID, "null argument");
    if (m->finalized) return fail(CP_ERR_STATE, "model already finalized");
    m->params[name] = std::vector<float>(host_data, host_data + numel);
    return CP_OK;
}

int cp_model_finalize(cp_model* m) {
    if (!m) return fail(CP_ERR_INVALID, "null model");
    if (m->finalized) return CP_OK;
    Packer pk{m};
    if (m->hourglass) pk.run_hourglass();
    else if (m->resnet) pk.run_resnet();
    else pk.run();
    pk.hip_ok(hipDeviceSynchronize());
    if (pk.status != CP_OK)
        return fail(pk.status, (pk.status == CP_ERR_STATE ? "missing or mis-shaped parameter: " : "finalize failed: ") + pk.missing);
    m->params.clear();
    m->finalized = true;
    return CP_OK;
}

void cp_model_destroy(cp_model* m) {
    if (!m) return;
    for (auto& r : m->prof) {
        (void)hipEventDestroy(r.e0);
        (void)hipEventDestroy(r.e1);
    }
    for (auto e : m->event_pool) (void)hipEventDestroy(e);
    for (auto& kv : m->graphs) (void)hipGraphExecDestroy(kv.second);
    for (void* p : m->device_allocs) (void)hipFree(p);
    delete m;
}

}  // extern "C"
