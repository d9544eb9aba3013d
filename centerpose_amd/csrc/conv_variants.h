// The kernel variants of the convolution launchers: one entry per template-instantiation family (what rocprofv3 lists as one kernel
// name) = enumerator, id, profile name.  The enum, cp_conv_variant_name's array and the count come from this list.  Ids and names are
// contract: tests/golden/engine_plan_pins.json, the files under profiles/ and tools/pmc_to_json.py hold them.  A new variant is one
// entry here (the next free id), one `case` in its launcher and one line in its selector (cp_conv_variant / cp_conv16_variant).
#pragma once
#define CP_CONV_VARIANT_TABLE(X)                                                                                              \
    X(IGEMM_N16, 0, "igemm_f32_16x16x4_m256n16") /* 0..13 exact f32 (igemm.hip) by N tile 16 / 32 / 64 / 128: plain conv */   \
    X(IGEMM_N32, 1, "igemm_f32_32x32x2_m256n32")                                                                              \
    X(IGEMM_N64, 2, "igemm_f32_32x32x2_m128n64")                                                                              \
    X(IGEMM_N128, 3, "igemm_f32_32x32x2_m128n128")                                                                            \
    X(DCN_IGEMM_N64, 4, "dcn_igemm_f32_32x32x2_m128n64") /* fused DCNv2 */                                                    \
    X(DCN_IGEMM_N128, 5, "dcn_igemm_f32_32x32x2_m128n128")                                                                    \
    X(IGEMM_CAT_N16, 6, "igemm_cat_f32_16x16x4_m256n16") /* over a virtual channel concat (Root) */                           \
    X(IGEMM_CAT_N32, 7, "igemm_cat_f32_32x32x2_m256n32")                                                                      \
    X(IGEMM_CAT_N64, 8, "igemm_cat_f32_32x32x2_m128n64")                                                                      \
    X(IGEMM_CAT_N128, 9, "igemm_cat_f32_32x32x2_m128n128")                                                                    \
    X(IGEMM_UNALIGNED_N16, 10, "igemm_unaligned_f32_16x16x4_m256n16") /* unaligned channels (7x7 stems) */                    \
    X(IGEMM_UNALIGNED_N32, 11, "igemm_unaligned_f32_32x32x2_m256n32")                                                         \
    X(IGEMM_UNALIGNED_N64, 12, "igemm_unaligned_f32_32x32x2_m128n64")                                                         \
    X(IGEMM_UNALIGNED_N128, 13, "igemm_unaligned_f32_32x32x2_m128n128")                                                       \
    X(IGEMM16_N32, 14, "igemm16_f16x3_m128n32") /* 14.. split-f16 "f16x3" (igemm16.hip) by N tile 32 / 64 / 128 */            \
    X(IGEMM16_N64, 15, "igemm16_f16x3_m128n64")                                                                               \
    X(IGEMM16_N128, 16, "igemm16_f16x3_m128n128")                                                                             \
    X(DCN16_N64, 17, "dcn_igemm16_f16x3_m128n64") /* dcn16.hip */                                                             \
    X(DCN16_N128, 18, "dcn_igemm16_f16x3_m128n128")                                                                           \
    X(IGEMM16_CAT_N32, 19, "igemm16_cat_f16x3_m128n32")                                                                       \
    X(IGEMM16_CAT_N64, 20, "igemm16_cat_f16x3_m128n64")                                                                       \
    X(IGEMM16_CAT_N128, 21, "igemm16_cat_f16x3_m128n128")                                                                     \
    X(FUSED_HEAD, 22, "igemm16_head_f16x3_m128n128")                                                                          \
    X(LOWC0, 23, "lowc_stem7x7_f16x3") /* lowc.hip by `kind`: 0 stem, 1 level0, 2 level1 */                                   \
    X(LOWC1, 24, "lowc_3x3_c16_f16x3")                                                                                        \
    X(LOWC2, 25, "lowc_3x3s2_c16_f16x3")                                                                                      \
    X(GRU, 26, "igemm16_gru_f16x3_m128n96")                                                                                   \
    X(HALO16_N32, 27, "halo16_f16x3_m128n32")                                                                                 \
    X(HALO16_N64, 28, "halo16_f16x3_m128n64")                                                                                 \
    X(HALO16_N128, 29, "halo16_f16x3_m128n128")                                                                               \
    X(DCN16P, 30, "dcn16p_f16x3_p128n64")                                                                                     \
    X(GN_FINAL, 31, "gn_final_f32_valu")                                                                                      \
    X(HALO_HEAD, 32, "halo16_head_f16x3_m128n128")                                                                            \
    X(HALO_GRU, 33, "halo16_gru_f16x3_m128n96")                                                                               \
    X(PW16_N64, 34, "pw16_f16x3_m128n64") /* pw16.hip: CoutPad % 128 != 0 / == 0 */                                           \
    X(PW16_N128, 35, "pw16_f16x3_m128n128")                                                                                   \
    X(DCN16S, 36, "dcn16s_f16x3_p128n64")                                                                                     \
    X(M64N64, 37, "igemm16_f16x3_m64n64")    /* igemm16p on 64 x 64 tiles (small launches) */                                 \
    X(DCN16PW, 38, "dcn16p_f16x3_p128n128")  /* dcn16p on the 128-wide N tile */                                              \
    X(DCN16T, 39, "dcn16t_f16x3_p128n64")                                                                                     \
    X(LOWC01, 40, "lowc_stem_level0_f16x3")  /* stem + level0 in one launch */                                                \
    X(STRM16, 41, "strm16_f16x3_w32n32")                                                                                      \
    X(LOWC1S, 42, "lowc_3x3s2_c16_rows_f16x3") /* level1 on the row-streaming kernel (kind 5) */                              \
    X(DECONV_F32, 43, "deconv16_f32_32x32x2_m256n64")                                                                         \
    X(DECONV16, 44, "deconv16_f16x3_m256n64")                                                                                 \
    X(HEAD_ROWS, 45, "igemm16_head_rows_f16x3_m128n128") /* fused head over a pixel list (heads at the decoded peaks) */
#define CP_NUM_CONV_VARIANTS 46
#define CP_X(name, id, str) CP_VARIANT_##name = id,
enum CpConvVariant : int { CP_VARIANT_NONE = -1, CP_CONV_VARIANT_TABLE(CP_X) };
#undef CP_X
#define CP_X(name, id, str) id,
constexpr int cp_variant_ids[] = {CP_CONV_VARIANT_TABLE(CP_X)};
#undef CP_X
constexpr bool cp_variant_ids_in_place(int i = 0) {
    return i == CP_NUM_CONV_VARIANTS || (cp_variant_ids[i] == i && cp_variant_ids_in_place(i + 1));
}
static_assert(sizeof(cp_variant_ids) / sizeof(int) == CP_NUM_CONV_VARIANTS, "CP_NUM_CONV_VARIANTS counts the table's entries");
static_assert(cp_variant_ids_in_place(), "entry i of the table has id i: cp_conv_variant_name indexes the names by id");

// A family's member by N tile (NONE: the family has no such tile; the DCN families run Cout <= 32 on their 64-wide tile)
struct CpVariantFamily { int n16, n32, n64, n128; };
constexpr CpVariantFamily CP_FAMILY_IGEMM = {CP_VARIANT_IGEMM_N16, CP_VARIANT_IGEMM_N32, CP_VARIANT_IGEMM_N64, CP_VARIANT_IGEMM_N128},
    CP_FAMILY_IGEMM_CAT = {CP_VARIANT_IGEMM_CAT_N16, CP_VARIANT_IGEMM_CAT_N32, CP_VARIANT_IGEMM_CAT_N64, CP_VARIANT_IGEMM_CAT_N128},
    CP_FAMILY_IGEMM_UNALIGNED = {CP_VARIANT_IGEMM_UNALIGNED_N16, CP_VARIANT_IGEMM_UNALIGNED_N32, CP_VARIANT_IGEMM_UNALIGNED_N64, CP_VARIANT_IGEMM_UNALIGNED_N128},
    CP_FAMILY_DCN_IGEMM = {CP_VARIANT_DCN_IGEMM_N64, CP_VARIANT_DCN_IGEMM_N64, CP_VARIANT_DCN_IGEMM_N64, CP_VARIANT_DCN_IGEMM_N128},
    CP_FAMILY_IGEMM16 = {CP_VARIANT_NONE, CP_VARIANT_IGEMM16_N32, CP_VARIANT_IGEMM16_N64, CP_VARIANT_IGEMM16_N128},
    CP_FAMILY_IGEMM16_CAT = {CP_VARIANT_NONE, CP_VARIANT_IGEMM16_CAT_N32, CP_VARIANT_IGEMM16_CAT_N64, CP_VARIANT_IGEMM16_CAT_N128},
    CP_FAMILY_DCN16 = {CP_VARIANT_DCN16_N64, CP_VARIANT_DCN16_N64, CP_VARIANT_DCN16_N64, CP_VARIANT_DCN16_N128},
    CP_FAMILY_HALO16 = {CP_VARIANT_NONE, CP_VARIANT_HALO16_N32, CP_VARIANT_HALO16_N64, CP_VARIANT_HALO16_N128},
    CP_FAMILY_PW16 = {CP_VARIANT_NONE, CP_VARIANT_NONE, CP_VARIANT_PW16_N64, CP_VARIANT_PW16_N128};
inline int cp_variant_for_tile(const CpVariantFamily& f, int bn) { return bn == 16 ? f.n16 : bn == 32 ? f.n32 : bn == 64 ? f.n64 : f.n128; }
inline bool cp_variant_is_pw16(int v) { return v == CP_VARIANT_PW16_N64 || v == CP_VARIANT_PW16_N128; }
inline bool cp_variant_is_halo16(int v) { return v == CP_VARIANT_HALO16_N32 || v == CP_VARIANT_HALO16_N64 || v == CP_VARIANT_HALO16_N128; }
