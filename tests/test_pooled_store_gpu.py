"""The 2x2 max-pooled copy a stride-2 level entry reads (Tree.downsample), written by the launch that produces the entry's input:
lowc1s_kernel for level 2's entry (lowc.hip, POOL), pw16s_kernel for the Root launches ahead of levels 3, 4 and 5 (pw16.hip, POOL).

dla_34 has four such entries; `<entry>.bottom` taps the pooled tensor in whichever form ran and cp_model_maxpool_launches counts
the stand-alone maxpool2 launches of the last pass.  A producer writes the copy when (engine_forward.hip: conv() / lowc(), pooled)
  * level1 runs on the row-streaming kernel (from 2048 wave jobs on, or CP_SEL_LEVEL1_ROWS_ALWAYS) and its output has even height
    and width;
  * a Root is a whole launch of pw16s_kernel -- f16x3, not CP_SEL_PW16_FRAG_A / _NEVER, at least 128 output tiles (below that the
    split-K plan takes the launch to 64 x 64 tiles or K slices) -- over a picture of even height and a width of whole 16-pixel blocks.
Shapes (B, H, W), the switches of the pass, the entries whose producer writes the copy, by that rule:
  * (4, 256, 256), LEVEL1_ROWS_ALWAYS: level1 (128 x 128), level2's root (M = 16384: 128 tiles, four 16-pixel blocks a row);
    level3's and level4's roots have 32 and 16 tiles and fall back.
  * (3, 256, 384), natural and LEVEL1_ROWS_ALWAYS: level2's root (64 x 96: six blocks a row, 144 tiles); level1 only when forced
    (288 wave jobs).
  * (16, 512, 512), natural: all four.
  * (2, 288, 288), natural: none -- level2's root is 72 pixels wide, the deeper ones 36 and 18.  (The engine takes multiples of
    32 only; this is the nearest such shape to one whose width at level 2 is no multiple of 16.)
max is exact, so the pooled tensor is torch.equal to F.max_pool2d of the producer's tap in either form, a Root's own output is
torch.equal to pw16_kernel's (CP_SEL_PW16_FRAG_A, whose epilogue is the plain one), and every head is torch.equal between the two
forms.  level1's row-streaming kernel has no bit-identical partner (the tile kernel sums in another order,
test_gpu_parity.py::test_row_streamed_level1_vs_tile_kernel_and_float64); its output is checked against that kernel to the same
4e-6 of the largest value."""
import pytest
import torch
import torch.nn.functional as F

from centerpose_amd import hip, synth

pytestmark = pytest.mark.gpu
S = hip.KernelSel
# entry, the tensor it reads
ENTRIES = [("base.level2", "base.level1"), ("base.level3", "base.level2"), ("base.level4", "base.level3"), ("base.level5", "base.level4")]
ROWS = S.LEVEL1_ROWS_ALWAYS
# (B, H, W), switches, entries (index into ENTRIES) whose producer writes the pooled copy
CASES = [((4, 256, 256), ROWS, {0, 1}), ((3, 256, 384), 0, {1}), ((3, 256, 384), ROWS, {0, 1}), ((16, 512, 512), 0, {0, 1, 2, 3}),
         ((2, 288, 288), 0, set())]

_cache = {}


def _model():
    if "m" not in _cache:
        heads = synth.HEADS_POSE
        _cache["m"] = hip.HipModel("dla_34", heads, synth.make_state_dict("dla_34", heads), precision="f16x3")
    return _cache["m"]


def _pass(model, x, sel, tap=None):
    """(heads or tap, maxpool2 launches, work space used, work space asked for) of one real pass"""
    with hip.select_kernels(sel):
        need = model.workspace_bytes(x.shape[0], x.shape[2], x.shape[3])
        if tap:
            out = model.forward(x, tap=tap)[1].clone()
        else:
            out = {k: v.clone() for k, v in model.forward(x).items()}
        torch.cuda.synchronize()
        return out, model.maxpool_launches(), model.workspace_used(), need


@pytest.mark.parametrize("shape,sel,pooled", CASES)
def test_pooled_copy_is_the_max_pool_of_the_producers_output(device, shape, sel, pooled):
    model = _model()
    B, H, W = shape
    x = synth.frames(B, seed=83, h=H, w=W).to(device)
    # the second form: every Root on pw16_kernel (maxpool2 launches for entries 3 .. 5), then level1 on the tile kernel as well
    frag = sel | S.PW16_FRAG_A
    none = (sel & ~S.LEVEL1_ROWS_ALWAYS) | S.PW16_FRAG_A | S.LEVEL1_ROWS_NEVER
    want = {sel: 4 - len(pooled), frag: 4 - len(pooled & {0}), none: 4}
    for form, n_want in want.items():
        _, n, used, need = _pass(model, x, form)
        print("%s switches %#x: maxpool2 launches %d (want %d), work space used %d of %d" % (shape, int(form), n, n_want, used, need))
        assert n == n_want, (shape, int(form), n, n_want)
        assert 0 < used <= need, (shape, int(form), used, need)
    for i, (entry, src) in enumerate(ENTRIES):
        prod, _, _, _ = _pass(model, x, sel, src)
        bottom, n, used, need = _pass(model, x, sel, entry + ".bottom")
        assert 0 < used <= need and float(prod.abs().max()) > 0
        ref = F.max_pool2d(prod, 2, 2)
        assert bottom.shape == ref.shape == (B, prod.shape[1], prod.shape[2] // 2, prod.shape[3] // 2)
        assert torch.equal(bottom, ref), (entry, float((bottom - ref).abs().max()))
        # the producer's own output: a Root against pw16_kernel, level1 against the tile kernel
        if i > 0:
            prod_f, _, _, _ = _pass(model, x, frag, src)
            assert torch.equal(prod, prod_f), (src, float((prod - prod_f).abs().max()))
            bottom_f, _, _, _ = _pass(model, x, frag, entry + ".bottom")
            assert torch.equal(bottom, bottom_f), entry
        else:
            prod_t, _, _, _ = _pass(model, x, none, src)
            top = max(1.0, float(prod_t.abs().max()))
            assert float((prod - prod_t).abs().max()) < 4e-6 * top, src


@pytest.mark.parametrize("shape,sel,pooled", CASES)
def test_heads_are_bit_identical_between_the_two_forms(device, shape, sel, pooled):
    model = _model()
    B, H, W = shape
    x = synth.frames(B, seed=89, h=H, w=W).to(device)
    xr = x.flip(0).contiguous()
    z0, _, _, _ = _pass(model, x, sel | S.PW16_FRAG_A)
    assert all(float(v.abs().max()) > 0 for v in z0.values())
    for it in range(10):
        for form in (sel, sel | S.PW16_FRAG_A):
            z, _, used, need = _pass(model, xr if it & 1 else x, form)
            assert 0 < used <= need
            for k in z0:
                zk = z[k].flip(0) if it & 1 else z[k]
                assert torch.equal(zk, z0[k]), (it, int(form), k)
