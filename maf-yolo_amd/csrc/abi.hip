// Signature table (include/mafyolo_hip.h, maf_abi_*): for every exported function its name and its signature as a string — one character for the
// return type, ':', one character per parameter — which the compiler derives from the prototype in the header, the way csrc/tape.hip derives its
// argument conversion.  A binding (maf-yolo_amd/lib.py) sets its argument and return types from this table instead of restating the header, so a
// changed prototype reaches it with the next build; a type the table cannot name stops the build here.  Host code only: no kernel lives here.
#include "maf_common.h"

namespace {

template <class T>
constexpr char kind_of() {
    if constexpr (std::is_void_v<T>) return 'v';                     // a return type only: no parameter has it
    else if constexpr (std::is_same_v<T, const char*>) return 's';   // a NUL-terminated string
    else if constexpr (std::is_pointer_v<T>) return 'p';             // any other pointer (maf_stream_t is void*)
    else if constexpr (std::is_same_v<T, float>) return 'f';
    else if constexpr (std::is_same_v<T, double>) return 'd';
    else if constexpr (std::is_same_v<T, int32_t>) return 'i';
    else if constexpr (std::is_same_v<T, int64_t>) return 'l';
    else static_assert(!sizeof(T), "the C-ABI passes pointers, float, double, int32_t and int64_t only: the binding has no conversion for this type");
}

template <class R, class... A>
struct Sig {
    static constexpr char str[] = {kind_of<R>(), ':', kind_of<A>()..., 0};
};

struct Entry {
    const char* name;
    const char* sig;
};

template <class R, class... A>
constexpr Entry entry(const char* name, R (*)(A...)) { return {name, Sig<R, A...>::str}; }

#define F(f) entry(#f, &f)

const Entry kEntries[] = {
    F(maf_abi_count), F(maf_abi_name), F(maf_abi_signature), F(maf_last_error), F(maf_version), F(maf_op_size), F(maf_op_launch),
    F(maf_engine_create), F(maf_engine_num_ops), F(maf_engine_run), F(maf_engine_run_filtered), F(maf_engine_run_graph), F(maf_engine_run_timed),
    F(maf_engine_destroy), F(maf_nms_workspace_bytes), F(maf_nms), F(maf_nms_ex), F(maf_nms_debug), F(maf_pack_w1x1_bytes), F(maf_pack_w1x1),
    F(maf_pack_dw), F(maf_pack_batch), F(maf_pack_desc_size), F(maf_ema_update), F(maf_ema_desc_size), F(maf_sgd_update), F(maf_sgd_desc_size),
    F(maf_nonfinite_check), F(maf_range_desc_size), F(maf_maxpool_forward), F(maf_maxpool_backward), F(maf_upsample2x_forward),
    F(maf_upsample2x_backward), F(maf_zero), F(maf_grad_fold), F(maf_add_sub2), F(maf_colsum), F(maf_dw_wgrad), F(maf_dw_wgrad31), F(maf_stem_train),
    F(maf_image_to_nhwc8), F(maf_bottleneck_record_bytes), F(maf_bottleneck_tail_record_bytes), F(maf_bottleneck_tail_supported),
    F(maf_conv1dw_record_bytes), F(maf_head_tail_record_bytes), F(maf_stem2_record_bytes), F(maf_conv3s2_lds_record_bytes),
    F(maf_mprep_lds_record_bytes), F(maf_mprep_wreg_record_bytes), F(maf_conv3s2_wreg_record_bytes), F(maf_conv1x1_stats_supported), F(maf_coco_rows),
    F(maf_conv1x1_wgrad), F(maf_conv_wgrad), F(maf_bn_forward), F(maf_bn_backward), F(maf_bn_backward_acc), F(maf_set_deterministic), F(maf_dw_branches),
    F(maf_dw_branches_stats), F(maf_bn_forward_ex), F(maf_bn_replicas), F(maf_bn_stats), F(maf_bn_sum_forward), F(maf_bn_sum_forward_stats),
    F(maf_bn_sum_backward), F(maf_tal_targets), F(maf_tal_assign), F(maf_atss_assign), F(maf_loss_partial_rows), F(maf_loss_decode), F(maf_loss_terms),
    F(maf_detect_join), F(maf_detect_join_backward), F(maf_nhwc_sum), F(maf_stream_fork), F(maf_stream_join), F(maf_tape_fn_id), F(maf_tape_fn_nargs),
    F(maf_tape_rec_size), F(maf_tape_run), F(maf_tape_toggle), F(maf_stream_create_masked), F(maf_stream_destroy), F(maf_letterbox),
    F(maf_letterbox_lds_bytes), F(maf_rescale_boxes), F(maf_augment_resize), F(maf_mosaic_affine), F(maf_augment_sample_size), F(maf_polygon_mask),
    F(maf_mosaic_affine_paste), F(maf_augment_paste_size), F(maf_area_struct_sizes), F(maf_resize_area), F(maf_pr_state_ints), F(maf_pr_out_doubles),
    F(maf_pr_workspace_bytes), F(maf_pr_match), F(maf_pr_curves), F(maf_coco_append), F(maf_coco_match), F(maf_coco_accumulate), F(maf_jpeg_struct_sizes),
    F(maf_jpeg_progressive_struct_sizes), F(maf_jpeg_decode), F(maf_jpeg_encode_struct_sizes), F(maf_jpeg_encode), F(maf_png_struct_sizes),
    F(maf_png_decode), F(maf_timer_create), F(maf_timer_start), F(maf_timer_stop), F(maf_timer_elapsed_ms), F(maf_timer_destroy),
};
constexpr int32_t kNumEntries = (int32_t)(sizeof(kEntries) / sizeof(kEntries[0]));

#undef F

}  // namespace

extern "C" int32_t maf_abi_count(void) { return kNumEntries; }
extern "C" const char* maf_abi_name(int32_t i) { return i >= 0 && i < kNumEntries ? kEntries[i].name : nullptr; }
extern "C" const char* maf_abi_signature(int32_t i) { return i >= 0 && i < kNumEntries ? kEntries[i].sig : nullptr; }
