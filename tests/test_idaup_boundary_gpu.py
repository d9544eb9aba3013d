"""ida_up's first up-sample + add inside the epilogue of dla_up.ida_2's last node (engine_forward.hip ida(): IdaNext).

The last node of dla_up.ida_2 (64 channels at 1/4 resolution) is read by one thing only: as `add` of ida_up's first iteration,
u_1 = up_1(proj_1(x[1])) + node.  x[1] is final once dla_up.ida_1 has run, so ida_up.proj_1 is launched before that node, the
node's dcn16t launch takes the up-sample + add epilogue (f = 2) and stores u_1; its own output and the upsample_add launch do not
exist.  Same conditions as inside an IDAUp (tests/test_upadd_epilogue_gpu.py): the node lands on dcn16t and no tap names the
node -- that very node, dla_up.ida_2.node_3, or its offset / mask map: a tap on another node runs the sites inside the IDAUps
unfused and leaves this one as it is.

Kernel pairing as there: fused = DCN16P_ALWAYS | DCN16T_ALWAYS against unfused = ... | DCN16S_ALWAYS | DCN16T_NEVER (dcn16s,
bit-identical to dcn16t).  upsample_add is not a profiled launch, so its count is not read here: what is counted is the nodes that
took an UpFuse, through the t bytes their dcn16t launches are charged for.  That a node with an UpFuse replaces the upsample_add
call of the iteration it feeds is ida()'s code (the only caller of upsample_add() sits in the branch a handed-over u skips), and
the kernel trace of the benchmark shows the launch gone (profiles/project_epilogue_kernel_stats_new.csv: 4 calls per step, the
parent's 5).  The sites -- a tap on the boundary node takes all four away (8 upsample_add launches, 4 fused), a tap on
another node the three inner ones (7)."""
import pytest
import torch

from centerpose_amd import hip, synth

pytestmark = pytest.mark.gpu
S = hip.KernelSel
FUSED = S.DCN16P_ALWAYS | S.DCN16T_ALWAYS
UNFUSED = S.DCN16P_ALWAYS | S.DCN16S_ALWAYS | S.DCN16T_NEVER
DCN16T = "dcn16t_f16x3_p128n64"


def _tap(model, x, name, sel):
    with hip.select_kernels(sel):
        _, t = model.forward(x, tap=name)
        return t.clone()


def _dcn16t_bytes(model, x, sel, tap=None):
    with hip.select_kernels(sel):
        model.profile(True)
        if tap is None:
            model.forward(x)
        else:
            model.forward(x, tap=tap)
        torch.cuda.synchronize()
        ran = model.profile_read()
        model.profile(False)
    return ran[DCN16T]["bytes"], ran[DCN16T]["launches"]


@pytest.mark.parametrize("B,H,W", [(2, 256, 512), (4, 320, 256)])
def test_boundary_fused_equals_unfused_bit_for_bit(device, B, H, W):
    heads = synth.HEADS_POSE
    sd = synth.make_state_dict("dla_34", heads)
    model = hip.HipModel("dla_34", heads, sd, precision="f16x3")
    x = synth.frames(B, seed=67, h=H, w=W).to(device)
    hf, wf = H // 4, W // 4
    # four fused sites, each charged for its t (64 channels): three at half the feature resolution (the boundary site among
    # them), one at a quarter; a tap on the boundary node runs all of them unfused on the same kernels, a tap on another node
    # all but the boundary site
    by_f, n_f = _dcn16t_bytes(model, x, FUSED)
    by_u, n_u = _dcn16t_bytes(model, x, FUSED, tap="dla_up.ida_2.node_3")
    by_i, n_i = _dcn16t_bytes(model, x, FUSED, tap="ida_up.node_1")
    t_inner = 4.0 * B * 64 * (2 * (hf // 2) * (wf // 2) + (hf // 4) * (wf // 4))
    t_boundary = 4.0 * B * 64 * (hf // 2) * (wf // 2)
    print("dcn16t launches %d / %d / %d, bytes fused - unfused = %.0f (inner sites %.0f + boundary %.0f), fused - inner unfused = %.0f" % (
        n_f, n_u, n_i, by_f - by_u, t_inner, t_boundary, by_f - by_i))
    assert n_f == n_u == n_i and abs((by_f - by_u) - (t_inner + t_boundary)) < 1.0 and abs((by_f - by_i) - t_inner) < 1.0
    # the mixed form (inner sites unfused, boundary fused) computes the same feature map
    assert torch.equal(_tap(model, x, "ida_up.node_2", FUSED), _tap(model, x, "feat", UNFUSED))
    for name in ("ida_up.up_1", "ida_up.proj_1", "feat"):
        a = _tap(model, x, name, FUSED)
        b = _tap(model, x, name, UNFUSED)
        assert float(a.abs().max()) > 0
        assert torch.equal(a, b), (name, float((a - b).abs().max()))
    u1 = _tap(model, x, "ida_up.up_1", FUSED)
    assert u1.shape == (B, 64, hf, wf)
    # the elided node: tapping it returns what the unfused sequence computes
    o_f = _tap(model, x, "dla_up.ida_2.node_3", FUSED)
    o_u = _tap(model, x, "dla_up.ida_2.node_3", UNFUSED)
    assert torch.equal(o_f, o_u)
    with hip.select_kernels(UNFUSED):
        z_u = {k: v.clone() for k, v in model.forward(x).items()}
    for it in range(20):
        for sel in (FUSED, UNFUSED):
            with hip.select_kernels(sel):
                z = model.forward(x)
                for k in z_u:
                    assert torch.equal(z[k], z_u[k]), (it, int(sel), k)
