"""Stand-in for the reference's pybind module ``_ext`` (DCNv2/src/vision.cpp:4-9): the forward and backward entry
points with the identical 14- and 15-argument signatures, routed to libcenterpose_hip.so.  The PS-ROI pooling ops are
unused by CenterPose and are not provided."""
from centerpose_amd import hip as _hip


def dcn_v2_forward(input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                   dilation_h, dilation_w, deformable_group):
    if not input.is_cuda:
        # dcn_v2.h:25-37 dispatches on the device; this build has the HIP path only
        raise RuntimeError("Not compiled with CPU support: centerpose_hip runs on the HIP device only")
    return _hip.dcn_v2_forward(input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w,
                               pad_h, pad_w, dilation_h, dilation_w, deformable_group)


def dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                    dilation_h, dilation_w, deformable_group):
    """[grad_input, grad_offset, grad_mask, grad_weight, grad_bias] (dcn_v2.h:48-80); the reference's semantics, including
    its input gradient's use of pad_h on both axes (include/centerpose_hip.h, cp_dcnv2_backward)."""
    if not input.is_cuda:
        raise RuntimeError("Not compiled with CPU support: centerpose_hip runs on the HIP device only")
    return _hip.dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w,
                                pad_h, pad_w, dilation_h, dilation_w, deformable_group)


def dcn_v2_backward_prec(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                         dilation_h, dilation_w, deformable_group, *, precision="f32"):
    """Not the reference's: ``dcn_v2_backward`` with the arithmetic of its two contractions as a keyword, "f32" or "f16x3"
    (``hip.ops.dcn_v2_backward``).  ``dcn_v2_backward`` itself keeps the reference's 15 arguments."""
    if not input.is_cuda:
        raise RuntimeError("Not compiled with CPU support: centerpose_hip runs on the HIP device only")
    return _hip.ops.dcn_v2_backward(input, weight, bias, offset, mask, grad_output, kernel_h, kernel_w, stride_h, stride_w,
                                    pad_h, pad_w, dilation_h, dilation_w, deformable_group, precision=precision)


def _not_built(*args, **kwargs):
    raise RuntimeError("centerpose_hip: PS-ROI pooling is not built (CenterPose does not use it)")


dcn_v2_psroi_pooling_forward = _not_built
dcn_v2_psroi_pooling_backward = _not_built
