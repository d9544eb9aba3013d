"""The binding's side of the lean detect path (no device needed): HipModel.detect's `heads` keyword, the LazyHeads mapping
(key order, lazy materialisation, stale-access error) with stubs in place of the model and the library, and the new entry
points in header <-> exported_symbols() <-> the built library."""
import inspect
import os
import re
from collections import OrderedDict

import pytest
import torch

from centerpose_amd import hip, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cp_model_lean_supported", "cp_model_detect_lean_workspace_bytes", "cp_model_detect_lean", "cp_model_dense_heads",
       "cp_model_heads_at_workspace_bytes", "cp_model_heads_at", "cp_decode_peaks_workspace_bytes", "cp_decode_peaks",
       "cp_decode_gathered"]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g

    g.build()
    return hip.lib()


def test_new_entry_points_are_declared_exported_and_resolve(built):
    header = open(os.path.join(REPO, "include", "centerpose_hip.h")).read()
    testing = open(os.path.join(REPO, "include", "centerpose_hip_testing.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in hip.exported_symbols()
        assert not re.search(r"\b%s\s*\(" % n, testing), n   # product ABI, not a test hook
        getattr(built, n)
    assert int(re.search(r"#define\s+CP_ABI_VERSION\s+(\d+)", header).group(1)) == 7
    nv = built.cp_num_kernel_variants()
    assert built.cp_kernel_variant_name(nv - 1).decode() == "igemm16_head_rows_f16x3_m128n128"


def test_sizes_and_refusals_are_host_arithmetic(built):
    assert built.cp_decode_peaks_workspace_bytes(2, 128, 128, 100) >= 256          # one-kernel peaks: no candidates
    big = built.cp_decode_peaks_workspace_bytes(2, 256, 256, 100)
    assert big >= 2 * 9 * 100 * 8                                                   # tiled: candidates per band
    assert built.cp_decode_peaks_workspace_bytes(1, 128, 126, 100) == 0            # W % 4
    assert built.cp_decode_peaks_workspace_bytes(1, 128, 128, 129) == 0            # K > 128
    assert built.cp_model_lean_supported(None, 1, 512, 512) == 0
    assert built.cp_model_detect_lean_workspace_bytes(None, 1, 512, 512, 100) == 0
    assert built.cp_model_heads_at_workspace_bytes(None, 1, 8) == 0
    assert built.cp_model_dense_heads(None, None, None) == -1


def test_detect_keyword():
    sig = inspect.signature(hip.HipModel.detect)
    assert sig.parameters["heads"].default == "lazy"
    assert list(sig.parameters)[:11] == ["self", "images", "pre_img", "pre_hm", "pre_hm_hp", "K", "rep_mode", "fit_gaussian",
                                          "balance", "legacy_bool_mask", "graph"]
    m = hip.HipModel.__new__(hip.HipModel)
    m._h = None
    with pytest.raises(ValueError):
        m.detect(torch.zeros(1, 3, 32, 32), heads="sparse")
    for word in ("lazy", "dense", "by-product", "raises"):
        assert word in hip.HipModel.detect.__doc__


class _StubModel(object):
    def __init__(self, gen):
        self._det_gen, self._h = gen, None


class _StubLib(object):
    def __init__(self):
        self.calls = 0

    def cp_model_dense_heads(self, h, stream, ptrs):
        self.calls += 1
        self.ptrs = list(ptrs)
        return 0


def _lazy(gen_model, gen_call):
    heads = synth.HEADS_POSE
    B, K, G = 2, 5, 8
    shapes = OrderedDict((k, (B, c, G, G)) for k, c in heads.items())
    ready = {k: torch.zeros(B, heads[k], G, G) for k in ("hm", "hm_hp")}
    gathered = OrderedDict((k, torch.zeros(*((B, 8, 2, K) if k == "hp_offset" else (B, c, K)))) for k, c in heads.items()
                           if k not in ("hm", "hm_hp"))
    return hip.LazyHeads(_StubModel(gen_model), gen_call, shapes, ready, gathered, torch.zeros(B, 9, K),
                         torch.zeros(B, 9, K, dtype=torch.int32)), heads


def test_lazy_heads_order_materialisation_and_stale_access(monkeypatch):
    stub = _StubLib()
    monkeypatch.setattr(hip._abi, "lib", lambda: stub)
    monkeypatch.setattr(hip._abi, "_stream", lambda: None)
    z, heads = _lazy(3, 3)
    assert list(z) == list(heads) == list(z.keys()) and len(z) == len(heads)
    assert "hps" in z and "nope" not in z
    with pytest.raises(KeyError):
        z["nope"]
    with pytest.raises(TypeError):
        z["hm"] = None                      # read-only
    assert z["hm"].shape == (2, 1, 8, 8) and z["hm_hp"].shape == (2, 8, 8, 8)
    assert stub.calls == 0 and not z.materialised()   # the heat-maps are there at once
    assert set(z.gathered) == set(heads) - {"hm", "hm_hp"} and z.gathered["hp_offset"].shape == (2, 8, 2, 5)
    assert z["wh"].shape == (2, 2, 8, 8)
    assert stub.calls == 1 and z.materialised()
    # one launch fills every remaining head; hm / hm_hp are not asked for again
    assert [p == 0 or p is None for p in stub.ptrs] == [k in ("hm", "hm_hp") for k in heads]
    for k, v in z.items():
        assert tuple(v.shape) == (2, heads[k], 8, 8)
    assert stub.calls == 1                  # cached
    # a later detect() on the model: the feature map is gone
    z2, _ = _lazy(4, 3)
    assert z2["hm"] is not None
    with pytest.raises(RuntimeError, match="next detect"):
        z2["hps"]
    with pytest.raises(RuntimeError, match="next detect"):
        list(z2.items())
    assert stub.calls == 1
