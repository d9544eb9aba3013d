"""The device-resident network (cp_model_*): ``HipModel`` and the ``LazyHeads`` mapping its lean detect path returns."""
import ctypes
from collections import OrderedDict
from collections.abc import Mapping
from ctypes import c_char_p, c_int, c_void_p

import torch

from . import _abi
from .detect import _MAP_HEADS, DET_STRIDE


class LazyHeads(Mapping):
    """What ``HipModel.detect(heads="lazy")`` returns for the heads on a model that takes the lean path: a read-only mapping
    with the model's head names in order.  ``hm`` / ``hm_hp`` are there at once.  Any other key -- also through ``items()`` /
    ``values()`` -- is the dense map the decode never needed: it is computed on first access from the feature map the detect
    call left behind (cp_model_dense_heads, on the current stream, all remaining heads in one launch) and cached.  After the
    next ``detect`` on the model that feature map is gone and such an access raises.
    ``gathered``: head -> compact table of the lean path ([B,C,K] at the centre peaks, hp_offset [B,8,2,K] at the joint
    peaks); ``pk_score`` / ``pk_ind``: the peaks [B,9,K]."""

    def __init__(self, model, gen, shapes, ready, gathered, pk_score, pk_ind):
        self._model, self._gen, self._shapes = model, gen, shapes
        self._ready = dict(ready)
        self.gathered, self.pk_score, self.pk_ind = gathered, pk_score, pk_ind

    def __iter__(self):
        return iter(self._shapes)

    def __len__(self):
        return len(self._shapes)

    def __contains__(self, k):   # (Mapping's own asks __getitem__, which would compute the maps)
        return k in self._shapes

    def __getitem__(self, k):
        if k not in self._shapes:
            raise KeyError(k)
        if k not in self._ready:
            self._materialise()
        return self._ready[k]

    def materialised(self):
        return len(self._ready) == len(self._shapes)

    def _materialise(self):
        m = self._model
        if m._det_gen != self._gen:
            raise RuntimeError("detect: the dense '%s' maps of this call were not read before the next detect() on the model, and "
                               "the feature map they are computed from is gone; read them earlier or call detect(heads=\"dense\")"
                               % "', '".join(k for k in self._shapes if k not in self._ready))
        dev = self.pk_ind.device
        new = OrderedDict((k, torch.empty(*shp, device=dev, dtype=torch.float32)) for k, shp in self._shapes.items()
                          if k not in self._ready)
        ptrs = (c_void_p * len(self._shapes))(*[new[k].data_ptr() if k in new else 0 for k in self._shapes])
        _abi._check(_abi.lib().cp_model_dense_heads(m._h, _abi._stream(), ptrs), "cp_model_dense_heads")
        self._ready.update(new)


class HipModel(object):
    """Device-resident DLA-34 / DLA-34+ConvGRU / hourglass / resdcn_N network built from a reference-format state dict."""

    def __init__(self, arch, heads, state_dict, tracking_task=False, head_conv=256, precision=None):
        L = _abi.lib()
        self.arch = arch
        self.heads = OrderedDict(heads)
        self.tracking_task = bool(tracking_task)
        names = (c_char_p * len(self.heads))(*[k.encode() for k in self.heads])
        classes = (c_int * len(self.heads))(*[int(v) for v in self.heads.values()])
        h = c_void_p()
        _abi._check(L.cp_model_create(arch.encode(), int(self.tracking_task), len(self.heads), names, classes,
                                      int(head_conv), ctypes.byref(h)), "cp_model_create")
        self._h = h
        for k, v in state_dict.items():
            if k.startswith("module.") and not k.startswith("module_list"):
                k = k[7:]  # lib/models/model.py:43-48
            if not torch.is_floating_point(v):
                continue  # num_batches_tracked
            t = v.detach().cpu().contiguous().float()
            _abi._check(L.cp_model_set_param(h, k.encode(), c_void_p(t.data_ptr()), t.numel()), "cp_model_set_param")
        _abi._check(L.cp_model_finalize(h), "cp_model_finalize")
        if precision is not None:
            self.set_precision(precision)
        self._ws = None

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and _abi._lib is not None:
                _abi._lib.cp_model_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_precision(self, name):
        _abi._check(_abi.lib().cp_model_set_precision(self._h, _abi.PRECISIONS[name]), "cp_model_set_precision")
        self.precision = name

    def profile(self, enable=True):
        """Arm / disarm per-launch HIP-event timing of the implicit-GEMM kernels."""
        _abi._check(_abi.lib().cp_model_profile(self._h, int(bool(enable))), "cp_model_profile")

    def _profile_table(self, n, read, what, name):
        buf = (ctypes.c_double * (n * 4))()
        _abi._check(read(self._h, buf, n), what)
        return OrderedDict((name(i).decode(), dict(launches=int(buf[i * 4]), ms=buf[i * 4 + 1], flops=buf[i * 4 + 2],
                                                   bytes=buf[i * 4 + 3])) for i in range(n) if buf[i * 4] > 0)

    def profile_read(self):
        """-> {kernel name: dict(launches, ms, flops, bytes)} accumulated since the last read."""
        L = _abi.lib()   # sized by the library, not by a copy of CP_NUM_KERNEL_VARIANTS
        return self._profile_table(L.cp_num_kernel_variants(), L.cp_model_profile_read, "cp_model_profile_read",
                                   L.cp_kernel_variant_name)

    def profile_roles(self):
        """-> {role: dict(launches, ms, flops, bytes)} of the launches drained by the last profile_read()."""
        L = _abi.lib()
        return self._profile_table(L.cp_num_roles(), L.cp_model_profile_roles, "cp_model_profile_roles", L.cp_role_name)

    def workspace_bytes(self, B, H, W):
        return self._sized("cp_model_workspace_bytes", B, H, W)

    def _sized(self, query, *shape):
        n = getattr(_abi.lib(), query)(self._h, *shape)
        if n == 0:
            raise RuntimeError(query + " failed: " + _abi.lib().cp_last_error().decode())
        return n

    def workspace_used(self):
        """Bytes of the work space the last pass reached (cp_model_workspace_used): at most workspace_bytes() of its shape."""
        return int(_abi.lib().cp_model_workspace_used(self._h))

    def maxpool_launches(self):
        """Stand-alone 2x2 max-pool launches of the last pass (cp_model_maxpool_launches): the stride-2 level entries whose pooled
        input was not written by its producer."""
        return int(_abi.lib().cp_model_maxpool_launches(self._h))

    @staticmethod
    def _fits(buf, nbytes, device):
        """The one rule for every work-space buffer the model keeps between calls: ``buf`` serves again only while it has exactly
        the size the library asks for now, on the same device.  What a shape needs also depends on the precision and on the
        kernel-selection switches, so every call asks (the library caches its answer) and no buffer outlives the size it was
        allocated for."""
        return buf is not None and buf.numel() == nbytes and buf.device == torch.device(device)

    def _workspace(self, B, H, W, device):
        need = self.workspace_bytes(B, H, W)
        if not self._fits(self._ws, need, device):
            self._ws = None   # (freed before its successor is allocated)
            self._ws = _abi._workspace(need, device)
        return self._ws

    def forward(self, images, pre_img=None, pre_hm=None, pre_hm_hp=None, sigmoid_hm=False, tap=None):
        """images [B,3,H,W] on the HIP device -> OrderedDict head -> [B,classes,H/4,W/4].
        With ``tap`` also returns the named intermediate activation as NCHW.  A tap changes the launch sequence: the fused heads
        are off, and a tap whose name contains ``.node_`` (an IDAUp node or its offset / mask map) runs every IDAUp with its
        stand-alone up-sample + add launches, so a profile taken with such a tap is that of the unfused sequence (the one site
        between two IDAUps, dla_up's last node storing ida_up's first sum, is unfused only by a tap on that node).  Likewise a tap on
        any level entry's ``<entry>.project`` runs every entry's projection as a launch of its own (it is otherwise computed inside the
        block's conv2 and never stored)."""
        L = _abi.lib()
        images = _abi._dev(images)
        B, _, H, W = images.shape
        inputs = _abi._ptrs(images, *map(_abi._dev_opt, (pre_img, pre_hm, pre_hm_hp)))
        outs = OrderedDict()
        for k, c in self.heads.items():
            outs[k] = torch.empty(B, c, H // 4, W // 4, device=images.device, dtype=torch.float32)
        ptrs = (c_void_p * len(outs))(*[t.data_ptr() for t in outs.values()])
        ws = self._workspace(B, H, W, images.device)
        if tap is None:
            rc = L.cp_model_forward(self._h, _abi._stream(), B, H, W, *inputs, ptrs, int(bool(sigmoid_hm)), _abi._ptr(ws),
                                    ws.numel())
            _abi._check(rc, "cp_model_forward")
            return outs
        tap_buf = torch.zeros(B * 16 * H * W, device=images.device, dtype=torch.float32)
        dims = (c_int * 3)(0, 0, 0)
        rc = L.cp_model_forward_tap(self._h, _abi._stream(), B, H, W, *inputs, ptrs, int(bool(sigmoid_hm)), _abi._ptr(ws),
                                    ws.numel(), tap.encode(), _abi._ptr(tap_buf), dims)
        _abi._check(rc, "cp_model_forward_tap")
        C, h, w = dims[0], dims[1], dims[2]
        if C == 0:
            raise RuntimeError("unknown tap %r" % tap)
        return outs, tap_buf[: B * C * h * w].view(B, C, h, w)

    def features(self, images, pre_img=None, pre_hm=None, pre_hm_hp=None):
        """The tensor the heads read (cp_model_features): images [B,3,H,W] -> [B,Cin,H/4,W/4] in channels_last memory format (the
        engine's NHWC buffer, no copy); no head is launched.  dla_34 and resdcn_* only."""
        L = _abi.lib()
        if self.arch.startswith("dlav1") or self.arch == "hourglass":
            raise NotImplementedError("features(): %s has no single feature map that plain conv3x3 -> ReLU -> conv1x1 heads read"
                                      % self.arch)
        images = _abi._dev(images)
        B, _, H, W = images.shape
        inputs = _abi._ptrs(images, *map(_abi._dev_opt, (pre_img, pre_hm, pre_hm_hp)))
        feat = torch.empty(B, H // 4, W // 4, 64, device=images.device, dtype=torch.float32)
        ws = self._workspace(B, H, W, images.device)
        rc = L.cp_model_features(self._h, _abi._stream(), B, H, W, *inputs, _abi._ptr(feat), _abi._ptr(ws), ws.numel())
        _abi._check(rc, "cp_model_features")
        return feat.permute(0, 3, 1, 2)

    def lean_supported(self, B, H, W):
        """Does detect(heads="lazy") take the lean path for this shape (cp_model_lean_supported)?"""
        return bool(_abi.lib().cp_model_lean_supported(self._h, int(B), int(H), int(W)))

    def heads_at(self, index):
        """The regression heads (every head but hm / hm_hp) at the pixels ``index`` [B,n] (int32, y * (W/4) + x) of the feature
        map the last lean detect() left behind -> OrderedDict head -> [B,classes,n] (cp_model_heads_at)."""
        L = _abi.lib()
        index = index.to(torch.int32).contiguous()
        B, n = index.shape
        out = OrderedDict((k, torch.empty(B, c, n, device=index.device, dtype=torch.float32)) for k, c in self.heads.items()
                          if k not in _MAP_HEADS)
        ptrs = (c_void_p * len(self.heads))(*[out[k].data_ptr() if k in out else 0 for k in self.heads])
        ws = _abi._workspace(max(L.cp_model_heads_at_workspace_bytes(self._h, B, n), 256), index.device)
        _abi._check(L.cp_model_heads_at(self._h, _abi._stream(), _abi._ptr(index), n, ptrs, _abi._ptr(ws), ws.numel()),
                    "cp_model_heads_at")
        return out

    def _detect_lean(self, images, pre_img, pre_hm, pre_hm_hp, K, rep_mode, fit_gaussian, balance, legacy_bool_mask, graph):
        L = _abi.lib()
        B, _, H, W = images.shape
        dev = images.device
        key = ("lean", B, H, W, str(dev), K)
        need = self._sized("cp_model_detect_lean_workspace_bytes", B, H, W, K)
        st = getattr(self, "_lean_state", None)
        if st is not None and (st[0] != key or not self._fits(st[6], need, dev)):
            st = self._lean_state = None   # (another shape, or the same one under another precision / switch setting)
        if st is None:
            f32 = dict(device=dev, dtype=torch.float32)
            maps = OrderedDict((k, torch.empty(B, self.heads[k], H // 4, W // 4, **f32)) for k in _MAP_HEADS)
            tables = OrderedDict((k, torch.empty(*((B, 8, 2, K) if k == "hp_offset" else (B, c, K)), **f32))
                                 for k, c in self.heads.items() if k not in _MAP_HEADS)
            pk_score = torch.empty(B, 9, K, **f32)
            pk_ind = torch.empty(B, 9, K, device=dev, dtype=torch.int32)
            det = torch.empty(B, K, DET_STRIDE, **f32)
            ws = _abi._workspace(need, dev)
            hp = (c_void_p * len(self.heads))(*[maps[k].data_ptr() if k in maps else 0 for k in self.heads])
            tp = (c_void_p * len(self.heads))(*[tables[k].data_ptr() if k in tables else 0 for k in self.heads])
            shapes = OrderedDict((k, (B, c, H // 4, W // 4)) for k, c in self.heads.items())
            st = (key, maps, tables, pk_score, pk_ind, det, ws, hp, tp, shapes)
            self._lean_state = st
        _, maps, tables, pk_score, pk_ind, det, ws, hp, tp, shapes = st
        rc = L.cp_model_detect_lean(self._h, _abi._stream(), B, H, W, *_abi._ptrs(images, pre_img, pre_hm, pre_hm_hp),
                                    hp, tp, _abi._ptr(pk_score), _abi._ptr(pk_ind), int(K), int(rep_mode), int(bool(fit_gaussian)),
                                    float(balance), int(bool(legacy_bool_mask)), _abi._ptr(det), _abi._ptr(ws), ws.numel(),
                                    int(bool(graph)))
        _abi._check(rc, "cp_model_detect_lean")
        return LazyHeads(self, self._det_gen, shapes, maps, tables, pk_score, pk_ind), det

    def detect(self, images, pre_img=None, pre_hm=None, pre_hm_hp=None, K=100, rep_mode=1, fit_gaussian=False,
               balance=2.0, legacy_bool_mask=False, graph=True, heads="lazy"):
        """backbone + heads + sigmoid + decode in one library call -> (heads mapping, det [B,K,118]).
        Output tensors are owned by the model and REUSED by the next call with the same batch shape (that is what lets
        the launch sequence be replayed from a hipGraph).  With ``graph`` the caller must run on a non-default stream
        and pass the same input tensors (copy new frames into them).

        The decode reads hm and hm_hp on every pixel, but the regression heads only at the decoded peaks: their dense maps
        are a by-product it never needed.  ``heads="lazy"`` (default), on a model that supports it (f16x3, grouped fused
        heads: dla_34, hourglass -- ``lean_supported``), runs cp_model_detect_lean, which evaluates those heads at the peaks
        only; the first return value is then a ``LazyHeads`` mapping (same keys, same order) whose regression maps are
        computed on first access, at their old cost, and only until the next ``detect`` on the model (afterwards such an
        access raises).  On any other model ``"lazy"`` is today's call and returns the plain OrderedDict.
        ``heads="dense"``: cp_model_detect, every map computed up front."""
        if heads not in ("lazy", "dense"):
            raise ValueError("detect: heads must be 'lazy' or 'dense'")
        L = _abi.lib()
        B, _, H, W = images.shape
        for t in (images, pre_img, pre_hm, pre_hm_hp):
            if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
                raise RuntimeError("detect: inputs must be contiguous float32 device tensors")
        self._det_gen = getattr(self, "_det_gen", 0) + 1   # (what a LazyHeads of an earlier call checks)
        if heads == "lazy" and L.cp_model_lean_supported(self._h, B, H, W):
            return self._detect_lean(images, pre_img, pre_hm, pre_hm_hp, K, rep_mode, fit_gaussian, balance, legacy_bool_mask,
                                     graph)
        key = ("det", B, H, W, str(images.device), K)
        need = self._sized("cp_model_detect_workspace_bytes", B, H, W, K)
        st = getattr(self, "_det_state", None)
        if st is not None and (st[0] != key or not self._fits(st[3], need, images.device)):
            st = self._det_state = None   # (another shape, or the same one under another precision / switch setting)
        if st is None:
            outs = OrderedDict((k, torch.empty(B, c, H // 4, W // 4, device=images.device, dtype=torch.float32))
                               for k, c in self.heads.items())
            det = torch.empty(B, K, DET_STRIDE, device=images.device, dtype=torch.float32)
            ws = _abi._workspace(need, images.device)
            ptrs = (c_void_p * len(outs))(*[t.data_ptr() for t in outs.values()])
            st = (key, outs, det, ws, ptrs)
            self._det_state = st
        _, outs, det, ws, ptrs = st
        rc = L.cp_model_detect(self._h, _abi._stream(), B, H, W, *_abi._ptrs(images, pre_img, pre_hm, pre_hm_hp),
                               ptrs, int(K), int(rep_mode), int(bool(fit_gaussian)), float(balance),
                               int(bool(legacy_bool_mask)), _abi._ptr(det), _abi._ptr(ws), ws.numel(), int(bool(graph)))
        _abi._check(rc, "cp_model_detect")
        return outs, det

    __call__ = forward
