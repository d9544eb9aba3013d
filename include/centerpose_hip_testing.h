/*
 * centerpose_hip_testing.h -- test hooks of libcenterpose_hip.so.  NOT part of the product ABI (centerpose_hip.h): nothing
 * in centerpose_amd/lib or bench.py's timed regions calls these; tests/ and the A/B tools under tools/ do.
 */
#ifndef CENTERPOSE_HIP_TESTING_H
#define CENTERPOSE_HIP_TESTING_H

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel SELECTION switches (process-global; 0 = the engine's own choice).  Every bit picks another implementation of the
 * same layer among the ones the library ships, so that the parity tests can compare two implementations on one input.
 * Every combination computes the layer correctly (to the summation-order round-off the tests state), except that
 * CP_SEL_NO_PRESCALE is correct only for inputs inside binary16's range (it exists for the range-safety tests:
 * tests/test_scale_equivariance_gpu.py, test_without_the_prescale_the_scaled_case_leaves_binary16, runs a model whose activations
 * sit 2^14 above synth's under it and requires the per-layer gate to fail).
 * cp_set_debug returns CP_ERR_INVALID, and keeps the current selection, when a bit outside CP_SEL_ALL is set.  Bit 11
 * (2048, once "alternative DCN wave counts") is unused and refused.
 * CP_SEL_PW16_FRAG_A and CP_SEL_PW16_NEVER also change the launch SEQUENCE of DLA's level entries: the entry's 1x1 projection,
 * by default computed inside the first block's conv2 with pw16s_kernel's arithmetic and never stored, is asked for on another
 * kernel and therefore runs as a launch of its own (same values; the parity tests' unfused reference).  Likewise the entries'
 * 2x2 max-pooled input, by default stored by the launch that produces the entry's input (pw16s_kernel for a Root, the
 * row-streaming level1 kernel): under these two switches, and under CP_SEL_LEVEL1_ROWS_NEVER for level 2's, it is made by a
 * maxpool2 launch (same values; cp_model_maxpool_launches counts them). */
#define CP_SEL_HEADS_SLABS 0x00000001          /* grouped fused heads write slabs + a reduction launch (no fuse_final) */
#define CP_SEL_HEADS_WG_PER_HEAD 0x00000002    /* grouped fused heads: one workgroup per (patch, head), not per patch */
#define CP_SEL_PW16_FRAG_A 0x00000004          /* 1x1 layers: fragment-shaped A loads (pw16_kernel), not staging rows */
#define CP_SEL_SPLITK_ELEMENTWISE 0x00000008   /* split-K epilogue element-wise, not the quad form */
#define CP_SEL_TILE128_SMALL 0x00000010        /* small launches on 128-row tiles, not 64 x 64 */
#define CP_SEL_NO_HEAD_FUSION 0x00000020       /* prediction heads as separate 3x3 and 1x1 layers */
#define CP_SEL_NO_LOWC 0x00000040              /* no lowc.hip kernels for the first layers */
#define CP_SEL_GN_HEAD_F32 0x00000080          /* GroupNorm'd heads' 1x1 on the exact-f32 kernel */
#define CP_SEL_GRU_UNFUSED 0x00000100          /* ConvGRU step without the fused gate epilogue */
#define CP_SEL_NO_PRESCALE 0x00000200          /* no activation |max| tracking / pre-scale of f16x3 operands */
#define CP_SEL_DCN16S_GRID8 0x00000400         /* dcn16s on 8 workgroups, so small launches walk several items each */
#define CP_SEL_HALO_NEVER 0x00001000           /* halo16 never (per-tap implicit GEMM instead) */
#define CP_SEL_HALO_ALWAYS 0x00002000          /* halo16 for every eligible N tile, not the 32-wide one only */
#define CP_SEL_HALO_LDS_WEIGHTS 0x00004000     /* LDS-staged weights in the halo16 kernels, not fragments from L2 */
#define CP_SEL_DCN16P_NEVER 0x00008000         /* patch-resident DCN kernels (dcn16p / s / t) never */
#define CP_SEL_DCN16P_ALWAYS 0x00010000        /* patch-resident DCN kernels for launches of any size */
#define CP_SEL_GN_HEAD_MFMA 0x00020000         /* GroupNorm'd heads' final 1x1 on the matrix cores, not gn_final_kernel */
#define CP_SEL_LEVEL1_ROWS_NEVER 0x00040000    /* level1 never on the row-streaming lowc kernel */
#define CP_SEL_DCN16P_NOT_WIDE 0x00080000      /* dcn16p never on the 128-wide N tile */
#define CP_SEL_DCN16S_NEVER 0x00100000         /* streamed DCN (dcn16s) never */
#define CP_SEL_DCN16S_ALWAYS 0x00200000        /* dcn16s for every eligible launch */
#define CP_SEL_PW16_NEVER 0x00400000           /* 1x1 layers on the LDS-staged loop, not pw16.hip */
#define CP_SEL_DCN_GENERIC 0x00800000          /* cp_dcnv2_forward always on the generic f32 kernel */
#define CP_SEL_HEADS_PER_HEAD_LAUNCH 0x01000000 /* fused heads one launch per head, not one grouped launch */
#define CP_SEL_DCN16T_ALWAYS 0x02000000        /* three-workgroup DCN (dcn16t) for every eligible launch */
#define CP_SEL_DCN16T_NEVER 0x04000000         /* dcn16t never */
#define CP_SEL_STEM_LEVEL0_UNFUSED 0x08000000  /* stem and level0 as two kernels, not the fused one */
#define CP_SEL_STRM16_NEVER 0x10000000         /* row-streamed 64 -> <= 32 channel 3x3 layers (strm16) never */
#define CP_SEL_STRM16_ALWAYS 0x20000000        /* strm16 for layers of any size */
#define CP_SEL_LEVEL1_ROWS_ALWAYS 0x40000000   /* level1 on the row-streaming lowc kernel at any size */
#define CP_SEL_ALL 0x7ffff7ff                  /* every defined switch */

int cp_set_debug(int flags);

#ifdef __cplusplus
}
#endif
#endif
