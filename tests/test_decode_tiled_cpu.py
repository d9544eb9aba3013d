"""CPU tests (no GPU) of the tiled decode's C ABI: cp_decode_tiled / cp_decode_tiled_workspace_bytes are exported and
bound, the workspace is pure host arithmetic that grows with the output grid, and every shape outside the envelope
(K <= 128, K <= H*W <= 1048576, W % 4 == 0, W <= 4096) or a short workspace is refused before anything is launched."""
import ctypes
import math

import pytest
import torch

from centerpose_amd import hip

TILE_PIX = 8192  # largest band of whole rows one workgroup of peaks_tile_kernel holds (decode.hip)


@pytest.fixture(scope="module")
def L():
    return hip.lib()


def _call(L, B, H, W, K, ws_bytes):
    """cp_decode_tiled with placeholder (never dereferenced) pointers: only the argument checks can run."""
    p = ctypes.c_void_p(4096)
    return L.cp_decode_tiled(None, B, H, W, p, p, p, None, None, None, None, p, None, None, None, K, 1, 0, 2.0, 0, 0, p,
                             p, ws_bytes)


def test_tiled_decode_symbols_are_exported_and_bound(L):
    for name in ("cp_decode_tiled_workspace_bytes", "cp_decode_tiled"):
        assert hasattr(L, name)
        assert name in hip.exported_symbols()
    assert hip.ABI_VERSION == L.cp_abi_version() == 7
    assert callable(hip.decode_raw_tiled)


def test_tiled_workspace_grows_with_the_grid(L):
    prev = 0
    for B, H, W in ((1, 128, 128), (1, 256, 256), (1, 488, 368), (1, 1024, 1024)):
        n = L.cp_decode_tiled_workspace_bytes(B, H, W, 100)
        assert n > prev
        prev = n
    for B, H, W, K in ((1, 128, 128, 100), (2, 488, 368, 100), (8, 488, 368, 128), (32, 256, 256, 1), (1, 2048, 4, 128),
                       (1, 1024, 1024, 128), (1, 255, 4100 - 4100 % 4 - 8, 128)):
        T = math.ceil(H * W / TILE_PIX)  # at least this many bands of whole rows
        n = L.cp_decode_tiled_workspace_bytes(B, H, W, K)
        assert n >= B * 9 * T * K * 8, (B, H, W, K, n)
        assert n >= L.cp_decode_workspace_bytes(B, K) - 256  # the peak table cp_decode keeps is part of it
    # batch scales the size linearly (up to the fixed alignment slack)
    one, eight = L.cp_decode_tiled_workspace_bytes(1, 488, 368, 100), L.cp_decode_tiled_workspace_bytes(8, 488, 368, 100)
    assert 7 * one < eight <= 8 * one


def test_decode_raw_tiled_has_no_cpu_path():
    with pytest.raises(RuntimeError):
        hip.decode_raw_tiled(torch.zeros(1, 1, 256, 256), torch.zeros(1, 16, 256, 256), torch.zeros(1, 2, 256, 256),
                             torch.zeros(1, 8, 256, 256))


@pytest.mark.parametrize("H,W,K,why", [
    (256, 258, 100, "W % 4"),
    (256, 256, 129, "K > 128"),
    (256, 256, 0, "K < 1"),
    (4, 8, 33, "H*W < K"),
    (1028, 1024, 100, "above 2^20 pixels"),
    (2, 8192, 100, "W > 4096"),
    (0, 256, 100, "empty grid"),
])
def test_tiled_decode_rejects_shapes_outside_the_envelope(L, H, W, K, why):
    assert L.cp_decode_tiled_workspace_bytes(1, H, W, K) == 0, why
    assert _call(L, 1, H, W, K, 1 << 30) == -1, why
    assert b"unsupported shape" in L.cp_last_error(), why


def test_tiled_decode_envelope_edges_are_accepted(L):
    for H, W, K in ((1024, 1024, 128), (256, 4096, 128), (2048, 4, 128), (1, 128, 128), (32, 4, 128)):
        assert L.cp_decode_tiled_workspace_bytes(1, H, W, K) > 0, (H, W, K)


def test_tiled_decode_rejects_short_workspace_and_bad_arguments(L):
    n = L.cp_decode_tiled_workspace_bytes(2, 488, 368, 100)
    assert _call(L, 2, 488, 368, 100, n - 1) == -1
    assert b"workspace too small" in L.cp_last_error()
    assert _call(L, 0, 488, 368, 100, n) == -1
    p = ctypes.c_void_p(4096)
    assert L.cp_decode_tiled(None, 1, 488, 368, None, p, p, None, None, None, None, p, None, None, None, 100, 1, 0, 2.0, 0,
                             0, p, p, n) == -1
    assert b"required" in L.cp_last_error()
    assert L.cp_decode_tiled(None, 1, 488, 368, p, p, p, None, None, None, None, p, None, None, None, 100, 5, 0, 2.0, 0,
                             0, p, p, n) == -1
    # the one-workgroup decode keeps its contract: 32768 pixels at most
    m = L.cp_decode_workspace_bytes(1, 100)
    assert L.cp_decode(None, 1, 488, 368, p, p, p, None, None, None, None, p, None, None, None, 100, 1, 0, 2.0, 0, 0, p, p,
                       m) == -1


def test_host_post_process_at_keep_res_geometry():
    """keep_res / fix_short give the crop extent s as [width, height]: the length fields scale by the affine's own factor
    (the reference's s / max(w, h) cannot broadcast there), the scalar extent of fix_res keeps the reference's rule."""
    import numpy as np

    from centerpose_amd.lib.utils.post_process import length_ratio, object_pose_post_process

    assert length_ratio(512.0, 128, 128) == 4.0
    assert length_ratio(600.0, 96, 160) == 600.0 / 160
    assert length_ratio(np.array([1472.0, 1952.0], np.float32), 368, 488) == 4.0
    rng = np.random.RandomState(0)
    widths = dict(bboxes=4, scores=1, kps=16, clses=1, obj_scale=3, obj_scale_uncertainty=3, tracking=2, tracking_hp=16,
                  kps_displacement_mean=16, kps_displacement_std=16, kps_heatmap_mean=16, kps_heatmap_std=16,
                  kps_heatmap_height=8)
    dets = {k: rng.rand(1, 5, w).astype(np.float32) for k, w in widths.items()}
    c, s = np.array([720.0, 960.0], np.float32), np.array([1472.0, 1952.0], np.float32)
    out = object_pose_post_process(dets, [c], [s], 488, 368, None, Inference=True)[0]
    assert len(out) == 5
    np.testing.assert_allclose(out[2]["kps_displacement_std"], dets["kps_displacement_std"][0, 2] * 4.0 * 0.32, rtol=1e-6)
    np.testing.assert_allclose(out[2]["tracking"], dets["tracking"][0, 2] * 4.0, rtol=1e-6)
