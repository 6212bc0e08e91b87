"""ctypes binding of liblightglue_mi355x.so (C-ABI in include/lightglue_mi355x.h).

The library is built in-tree by ``make -C cs566-project-lightglue_amd/csrc`` (or
``__graft_entry__.build()``).  There is no fallback: if the library is missing or fails to load,
every entry point raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LIGHTGLUE_MI355X_LIB", os.path.join(_HERE, "liblightglue_mi355x.so"))
ABI_VERSION = 12

LG_OK, LG_E_INVALID, LG_E_HIP, LG_E_WEIGHTS, LG_E_WORKSPACE, LG_E_INTERNAL = 0, -1, -2, -3, -4, -5

EXPORTED_SYMBOLS = [
    "lg_abi_version",
    "lg_last_error",
    "lg_create",
    "lg_destroy",
    "lg_weight_count",
    "lg_weight_name",
    "lg_weight_numel",
    "lg_load_weights",
    "lg_workspace_bytes",
    "lg_forward",
    "lg_filter_workspace_bytes",
    "lg_filter_matches",
    "lg_sinkhorn_workspace_bytes",
    "lg_log_optimal_transport",
    # ragged batches (per-pair counts) for the Sinkhorn head, the filter and SuperGlue (ABI 12, additive)
    "lg_filter_matches_ragged",
    "lg_log_optimal_transport_ragged",
    "lg_sinkhorn_rerun_count",
    "lg_sinkhorn_force_exact",
    "sg_forward_ragged",
    "lg_profile_enable",
    "lg_profile_read",
    "lg_attention_workspace_bytes",
    "lg_attention",
    # kernel-level linear GEMM entry (ABI 12, no handle)
    "lg_linear_workspace_bytes",
    "lg_linear",
    "lg_plane_roundtrip",
    # kernel-level SuperPoint convolution and dense-head entries (ABI 12, no handle)
    "sp_conv_layer_workspace_bytes",
    "sp_conv_layer_rows",
    "sp_conv_layer",
    "sp_head_scores",
    "sp_head_normalize",
    # kernel-level assignment entry (ABI 12, no handle)
    "lg_assign_workspace_bytes",
    "lg_assign",
    "lg_assignment_workspace_bytes",
    "lg_assignment_head",
    # homography ground truth (ABI 12, no handle)
    "lg_gt_homography_workspace_bytes",
    "lg_gt_matches_from_homography",
    # pose-and-depth ground truth (ABI 12, no handle)
    "lg_gt_depth_workspace_bytes",
    "lg_gt_matches_from_pose_depth",
    # line ground truth from a homography and the batched assignment solver (ABI 12, no handle)
    "lg_gt_line_thresholds",
    "lg_gt_line_counts_workspace_bytes",
    "lg_gt_line_counts_homography",
    "lg_gt_line_labels_workspace_bytes",
    "lg_gt_line_labels",
    "lg_linear_sum_assignment_workspace_bytes",
    "lg_linear_sum_assignment",
    # line ground truth from pose and depth (ABI 12, no handle)
    "lg_gt_line_depth_thresholds",
    "lg_gt_line_counts_pose_depth_workspace_bytes",
    "lg_gt_line_counts_pose_depth",
    "lg_gt_line_labels_visibility_workspace_bytes",
    "lg_gt_line_labels_visibility",
    # nearest-neighbour matcher (ABI 12, no handle)
    "lg_nn_workspace_bytes",
    "lg_nn_match",
    # batched match evaluation (ABI 12, no handle)
    "lg_eval_matches",
    # batched robust homography estimation (ABI 12, no handle)
    "lg_ransac_lds_matches",
    "lg_ransac_homography",
    # batched robust homography estimation from point and line matches (ABI 12, no handle)
    "lg_ransac_lines_lds_capacity",
    "lg_ransac_homography_lines",
    # batched robust relative pose and its five-point solver alone (ABI 12, no handle)
    "lg_ransac_relpose",
    "lg_essential_5pt",
    # training (backward pass)
    "lg_train_saved_bytes",
    "lg_train_saved_bytes_ex",
    "lg_train_scratch_bytes",
    "lg_train_forward",
    "lg_train_backward",
    "lg_head_scratch_bytes",
    "lg_head_backward",
    "lg_head_backward_from_forward",
    "lg_head_nll_forward",
    "lg_head_nll_backward",
    "lg_head_forward",
    "lg_train_gemm_workspace_bytes",
    "lg_train_gemm",
    "lg_train_gemm_ex",
    "lg_train_attention",
    "lg_train_attention_backward",
    # SuperPoint extractor (include/superpoint_mi355x.h)
    "sp_create",
    "sp_open_create",
    "sp_destroy",
    "sp_weight_count",
    "sp_weight_name",
    "sp_weight_numel",
    "sp_load_weights",
    "sp_workspace_bytes",
    "sp_forward",
    "sp_sample_descriptors",
    # ALIKED extractor (include/aliked_mi355x.h; ABI 12, additive)
    "sp_aliked_create",
    "sp_aliked_destroy",
    "sp_aliked_weight_count",
    "sp_aliked_weight_name",
    "sp_aliked_weight_numel",
    "sp_aliked_load_weights",
    "sp_aliked_workspace_bytes",
    "sp_aliked_forward",
    "sp_aliked_deform_conv",
    "sp_aliked_set_profile",
    "sp_aliked_stage_ms",
    # GlueStick point-and-line matcher (include/gluestick_mi355x.h; ABI 12, additive)
    "sg_gluestick_create",
    "sg_gluestick_destroy",
    "sg_gluestick_weight_count",
    "sg_gluestick_weight_name",
    "sg_gluestick_weight_numel",
    "sg_gluestick_load_weights",
    "sg_gluestick_workspace_bytes",
    "sg_gluestick_forward",
    "sg_gluestick_line_update",
    "sg_gluestick_double_softmax",
    "sg_gluestick_line_scores",
    # wireframe step in front of GlueStick (include/wireframe_mi355x.h; ABI 12, additive, no handle)
    "lg_wireframe_workspace_bytes",
    "lg_wireframe_forward",
    "lg_wireframe_connectivity",
    "lg_sample_descriptors_corner",
    "sg_create",
    "sg_destroy",
    "sg_weight_count",
    "sg_weight_name",
    "sg_weight_numel",
    "sg_load_weights",
    "sg_workspace_bytes",
    "sg_forward",
    "sg_nll_loss",
    "sg_nll_workspace_bytes",
    "sg_nll_loss_ws",
    # data-parallel training (ABI 8)
    "lg_set_grad_ready_hook",
    "sg_collective_floats",
    "sg_set_collective",
    "sg_set_grad_ready_hook",
    # SuperGlue training
    "sg_train_saved_bytes",
    "sg_train_saved_tensor",
    "sg_train_scratch_bytes",
    "sg_train_forward",
    "sg_train_backward",
    "sg_nll_backward",
]
KERNEL_IDS = {"attention": 0, "gemm": 1, "assign": 2}
# lg_config_t.precision (include/lightglue_mi355x.h): "auto" = fp16x3 (device-side range scaling)
PRECISIONS = {"auto": 0, "bf16x6": 1}
# flag on "auto" (LG_PREC_ATTN_F16): the eval forward's attention in half precision, conf "flash"
PREC_ATTN_F16 = 0x100
# lg_outputs_t.precision_used -> LightGlue.last_precision_used
# flag on "auto" (LG_PREC_GEMM_F16): the eval forward's trunk linears in half precision, conf "mp"
PREC_GEMM_F16 = 0x400
PRECISION_NAMES = {0: "fp16x3", 1: "bf16x6", PREC_ATTN_F16: "fp16x3+fp16attn", PREC_GEMM_F16: "fp16gemm",
                   PREC_GEMM_F16 | PREC_ATTN_F16: "fp16gemm+fp16attn"}


class LGConfig(ctypes.Structure):
    _fields_ = [
        ("input_dim", ctypes.c_int32),
        ("descriptor_dim", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("num_heads", ctypes.c_int32),
        ("add_scale_ori", ctypes.c_int32),
        ("depth_confidence", ctypes.c_double),
        ("width_confidence", ctypes.c_double),
        ("filter_threshold", ctypes.c_double),
        ("precision", ctypes.c_int32),
    ]


_P = ctypes.c_void_p
# data-parallel training callbacks (include/lightglue_mi355x.h lg_grad_ready_fn, superglue_mi355x.h
# sg_grad_ready_fn / sg_collective_fn): keep the Python objects alive while registered
LG_GRAD_READY_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p)
SG_GRAD_READY_FN = LG_GRAD_READY_FN
SG_COLLECTIVE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p)


def fnptr(cb):
    """A registered callback as the C function pointer (None -> NULL: unregister)."""
    return None if cb is None else ctypes.cast(cb, ctypes.c_void_p)


class LGInputs(ctypes.Structure):
    _fields_ = [
        ("B", ctypes.c_int32),
        ("M", ctypes.c_int32),
        ("N", ctypes.c_int32),
        ("keypoints0", _P),
        ("keypoints1", _P),
        ("descriptors0", _P),
        ("descriptors1", _P),
        ("image_size0", _P),
        ("image_size1", _P),
        ("scales0", _P),
        ("oris0", _P),
        ("scales1", _P),
        ("oris1", _P),
        ("flags", ctypes.c_int32),
        # ABI 11: per-pair keypoint counts of a ragged batch, device int32 [B]; NULL = every slot full
        ("num_keypoints0", _P),
        ("num_keypoints1", _P),
    ]


LG_FWD_TRAINING_GATE = 1  # lg_inputs_t.flags: training mode, no early stop / pruning
LG_FWD_CHECKPOINTED = 2  # lg_inputs_t.flags: training keeps layer outputs only, backward recomputes (ABI 9)


class LGOutputs(ctypes.Structure):
    _fields_ = [
        ("matches0", _P),
        ("matches1", _P),
        ("matching_scores0", _P),
        ("matching_scores1", _P),
        ("log_assignment", _P),
        ("ref_descriptors0", _P),
        ("ref_descriptors1", _P),
        ("prune0", _P),
        ("prune1", _P),
        ("layer_descriptors0", _P),
        ("layer_descriptors1", _P),
        ("kept", _P),
        ("stop", _P),
        ("stop_layer", ctypes.c_int32),
        ("kept0", ctypes.c_int32),
        ("kept1", ctypes.c_int32),
        ("precision_used", ctypes.c_int32),
        ("similarity", _P),
    ]


LIN_EPI = {"store": 0, "qkv_rot": 1, "cross_qkv": 2, "ln_gelu": 3}  # LG_LIN_*


class LGLinearArgs(ctypes.Structure):  # lg_linear_args_t
    _fields_ = [
        ("R", ctypes.c_int32),
        ("K0", ctypes.c_int32),
        ("K", ctypes.c_int32),
        ("Nout", ctypes.c_int32),
        ("A0", _P),
        ("lda0", ctypes.c_int32),
        ("A1", _P),
        ("lda1", ctypes.c_int32),
        ("W", _P),
        ("bias", _P),
        ("res", _P),
        ("res2", _P),
        ("res2_row0", ctypes.c_int32),
        ("ldr", ctypes.c_int32),
        ("out_scale", ctypes.c_float),
        ("relu", ctypes.c_int32),
        ("precision", ctypes.c_int32),
        ("epi", ctypes.c_int32),
        ("ln_route", ctypes.c_int32),
        ("ln_g", _P),
        ("ln_b", _P),
        ("B", ctypes.c_int32),
        ("H", ctypes.c_int32),
        ("M", ctypes.c_int32),
        ("N", ctypes.c_int32),
        ("cosb", _P),
        ("sinb", _P),
        ("qk_scale", ctypes.c_float),
        ("mask_B", ctypes.c_int32),
        ("mask_M0", ctypes.c_int32),
        ("mask_N0", ctypes.c_int32),
        ("cnt", _P),
        ("sel", _P),
        ("sel_eq", ctypes.c_int32),
        ("poison", ctypes.c_int32),
        ("want_planes", ctypes.c_int32),
        ("Y", _P),
        ("Y2", _P),
        ("y2_row0", ctypes.c_int32),
        ("ldy", ctypes.c_int32),
        ("yp", _P),
        ("yp_rows", _P),
        ("q", _P),
        ("kp", _P),
        ("vp", _P),
        ("pstride", ctypes.c_int64),
        ("exp_a0", ctypes.c_int32),
        ("exp_a1", ctypes.c_int32),
        ("exp_out", ctypes.c_int32),
        ("exp_out_v", ctypes.c_int32),
        ("max_out", ctypes.c_float),
        ("max_out_v", ctypes.c_float),
        ("bound_out", ctypes.c_float),
    ]


class SPConvLayerArgs(ctypes.Structure):  # sp_conv_layer_args_t
    _fields_ = [
        ("B", ctypes.c_int32),
        ("H", ctypes.c_int32),
        ("W", ctypes.c_int32),
        ("Cin", ctypes.c_int32),
        ("Cout", ctypes.c_int32),
        ("pool", ctypes.c_int32),
        ("conv1a", ctypes.c_int32),
        ("x", _P),
        ("w", _P),
        ("bias", _P),
        ("post_scale", _P),
        ("post_shift", _P),
        ("y_rows", _P),
        ("y_planes", _P),
        ("exp_in", ctypes.POINTER(ctypes.c_int32)),
        ("exp_out", ctypes.POINTER(ctypes.c_int32)),
        ("max_out", ctypes.POINTER(ctypes.c_float)),
    ]


class SPConfig(ctypes.Structure):  # sp_config_t
    _fields_ = [
        ("has_detector", ctypes.c_int32),
        ("has_descriptor", ctypes.c_int32),
        ("descriptor_dim", ctypes.c_int32),
        ("nms_radius", ctypes.c_int32),
        ("refinement_radius", ctypes.c_int32),
        ("remove_borders", ctypes.c_int32),
        ("legacy_sampling", ctypes.c_int32),
        ("detection_threshold", ctypes.c_float),
    ]


class SPOpenConfig(ctypes.Structure):  # sp_open_config_t
    _fields_ = [
        ("descriptor_dim", ctypes.c_int32),
        ("nms_radius", ctypes.c_int32),
        ("remove_borders", ctypes.c_int32),
        ("detection_threshold", ctypes.c_float),
    ]


class SPInputs(ctypes.Structure):  # sp_inputs_t
    _fields_ = [
        ("B", ctypes.c_int32),
        ("C", ctypes.c_int32),
        ("H", ctypes.c_int32),
        ("W", ctypes.c_int32),
        ("image", _P),
        ("image_size", _P),
        ("max_keypoints", ctypes.c_int32),
        ("sparse", ctypes.c_int32),
    ]


class SPOutputs(ctypes.Structure):  # sp_outputs_t
    _fields_ = [
        ("dense_scores", _P),
        ("dense_descriptors", _P),
        ("capacity", ctypes.c_int32),
        ("keypoints", _P),
        ("keypoint_scores", _P),
        ("descriptors", _P),
        ("counts", _P),
        ("host_counts", _P),
    ]


class AlikedConfig(ctypes.Structure):  # sp_aliked_config_t
    _fields_ = [
        ("c1", ctypes.c_int32),
        ("c2", ctypes.c_int32),
        ("c3", ctypes.c_int32),
        ("c4", ctypes.c_int32),
        ("dim", ctypes.c_int32),
        ("M", ctypes.c_int32),
        ("nms_radius", ctypes.c_int32),
        ("max_num_keypoints", ctypes.c_int32),
        ("detection_threshold", ctypes.c_float),
    ]


class AlikedInputs(ctypes.Structure):  # sp_aliked_inputs_t
    _fields_ = [
        ("B", ctypes.c_int32),
        ("H", ctypes.c_int32),
        ("W", ctypes.c_int32),
        ("image", _P),
        ("image_size", _P),
    ]


class AlikedOutputs(ctypes.Structure):  # sp_aliked_outputs_t
    _fields_ = [
        ("score_map", _P),
        ("capacity", ctypes.c_int32),
        ("keypoints", _P),
        ("descriptors", _P),
        ("sampled_scores", _P),
        ("dispersity", _P),
        ("counts", _P),
        ("host_counts", _P),
    ]


SG_MAX_LAYERS = 64
SG_MAX_KENC = 7


class SGConfig(ctypes.Structure):  # sg_config_t
    _fields_ = [
        ("descriptor_dim", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("layer_types", ctypes.c_int32 * SG_MAX_LAYERS),
        ("n_kenc", ctypes.c_int32),
        ("keypoint_encoder", ctypes.c_int32 * SG_MAX_KENC),
        ("use_scores", ctypes.c_int32),
        ("sinkhorn_iterations", ctypes.c_int32),
        ("filter_threshold", ctypes.c_float),
    ]


class SGInputs(ctypes.Structure):  # sg_inputs_t
    _fields_ = [
        ("B", ctypes.c_int32),
        ("M", ctypes.c_int32),
        ("N", ctypes.c_int32),
        ("keypoints0", _P),
        ("keypoints1", _P),
        ("descriptors0", _P),
        ("descriptors1", _P),
        ("scores0", _P),
        ("scores1", _P),
        ("image_size0", _P),
        ("image_size1", _P),
        ("image_w0", ctypes.c_int32),
        ("image_h0", ctypes.c_int32),
        ("image_w1", ctypes.c_int32),
        ("image_h1", ctypes.c_int32),
    ]


class SGOutputs(ctypes.Structure):  # sg_outputs_t
    _fields_ = [
        ("matches0", _P),
        ("matches1", _P),
        ("matching_scores0", _P),
        ("matching_scores1", _P),
        ("sinkhorn_cost", _P),
        ("log_assignment", _P),
        ("descriptors0", _P),
        ("descriptors1", _P),
    ]


SG_GLUESTICK_MAX_LINE_ITERS = 16


class GSConfig(ctypes.Structure):  # sg_gluestick_config_t
    _fields_ = [
        ("descriptor_dim", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("layer_types", ctypes.c_int32 * SG_MAX_LAYERS),
        ("n_kenc", ctypes.c_int32),
        ("keypoint_encoder", ctypes.c_int32 * SG_MAX_KENC),
        ("num_line_iterations", ctypes.c_int32),
        ("filter_threshold", ctypes.c_float),
    ]


class GSInputs(ctypes.Structure):  # sg_gluestick_inputs_t
    _fields_ = [
        ("B", ctypes.c_int32),
        ("M", ctypes.c_int32),
        ("N", ctypes.c_int32),
        ("L0", ctypes.c_int32),
        ("L1", ctypes.c_int32),
        ("keypoints0", _P),
        ("keypoints1", _P),
        ("descriptors0", _P),
        ("descriptors1", _P),
        ("scores0", _P),
        ("scores1", _P),
        ("image_size0", _P),
        ("image_size1", _P),
        ("image_w0", ctypes.c_int32),
        ("image_h0", ctypes.c_int32),
        ("image_w1", ctypes.c_int32),
        ("image_h1", ctypes.c_int32),
        ("lines0", _P),
        ("lines1", _P),
        ("lines_junc_idx0", _P),
        ("lines_junc_idx1", _P),
        ("line_scores0", _P),
        ("line_scores1", _P),
    ]


class GSOutputs(ctypes.Structure):  # sg_gluestick_outputs_t
    _fields_ = [
        ("matches0", _P),
        ("matches1", _P),
        ("matching_scores0", _P),
        ("matching_scores1", _P),
        ("log_assignment", _P),
        ("descriptors0", _P),
        ("descriptors1", _P),
        ("line_log_assignment", _P),
        ("line_matches0", _P),
        ("line_matches1", _P),
        ("line_matching_scores0", _P),
        ("line_matching_scores1", _P),
        ("raw_line_scores", _P),
    ]


LG_WIREFRAME_MAX_LINES, LG_WIREFRAME_MAX_DIM = 2048, 1024


class WFConfig(ctypes.Structure):  # lg_wireframe_config_t
    _fields_ = [
        ("nms_radius", ctypes.c_double),
        ("merge_points", ctypes.c_int32),
        ("merge_line_endpoints", ctypes.c_int32),
        ("force_num_keypoints", ctypes.c_int32),
        ("force_num_lines", ctypes.c_int32),
        ("s", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class WFInputs(ctypes.Structure):  # lg_wireframe_inputs_t
    _fields_ = [
        ("B", ctypes.c_int32),
        ("L", ctypes.c_int32),
        ("K", ctypes.c_int32),
        ("J", ctypes.c_int32),
        ("D", ctypes.c_int32),
        ("Hc", ctypes.c_int32),
        ("Wc", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("lines", _P),
        ("line_scores", _P),
        ("keypoints", _P),
        ("keypoint_scores", _P),
        ("descriptors", _P),
        ("dense", _P),
        ("fill_junctions", _P),
        ("fill_keypoints", _P),
    ]


class WFOutputs(ctypes.Structure):  # lg_wireframe_outputs_t
    _fields_ = [
        ("points", _P),
        ("scores", _P),
        ("descriptors", _P),
        ("lines", _P),
        ("lines_junc_idx", _P),
        ("counts", _P),
        ("removed", _P),
        ("connectivity", _P),
        ("pl_associativity", _P),
    ]


ASSIGN_ROUTES = {"materialised": 0, "recomputed": 1}  # LG_ASSIGN_*
ASSIGN_SENTINEL_F, ASSIGN_SENTINEL_I = -123.456, -77  # LG_ASSIGN_SENTINEL_F (as fp32) / _I


class LGAssignArgs(ctypes.Structure):  # lg_assign_args_t
    _fields_ = [
        ("B", ctypes.c_int32),
        ("M", ctypes.c_int32),
        ("N", ctypes.c_int32),
        ("md0", _P),
        ("md1", _P),
        ("sim", _P),
        ("z0", _P),
        ("z1", _P),
        ("Mb", _P),
        ("Nb", _P),
        ("fixed", ctypes.c_int32),
        ("raw_counts", ctypes.c_int32),
        ("threshold", ctypes.c_float),
        ("route", ctypes.c_int32),
        ("poison", ctypes.c_int32),
        ("la", _P),
        ("m0", _P),
        ("m1", _P),
        ("s0", _P),
        ("s1", _P),
        ("exp_md", ctypes.c_int32),
        ("max_md", ctypes.c_float),
    ]


class LightGlueLibError(RuntimeError):
    pass


_lib = None


def load():
    """Load (once) and type the C-ABI library.  Raises if it is missing: no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LightGlueLibError(
            f"HIP library not found at {LIB_PATH}; build it with `make -C cs566-project-lightglue_amd/csrc` "
            "(or __graft_entry__.build())"
        )
    lib = ctypes.CDLL(LIB_PATH)
    sz = ctypes.c_size_t
    i32 = ctypes.c_int32
    sig = {
        "lg_abi_version": (ctypes.c_int, []),
        "lg_last_error": (ctypes.c_char_p, []),
        "lg_create": (ctypes.c_int, [ctypes.POINTER(LGConfig), ctypes.c_int, ctypes.POINTER(_P)]),
        "lg_destroy": (ctypes.c_int, [_P]),
        "lg_weight_count": (ctypes.c_int, [_P]),
        "lg_weight_name": (ctypes.c_char_p, [_P, ctypes.c_int]),
        "lg_weight_numel": (ctypes.c_int64, [_P, ctypes.c_int]),
        "lg_load_weights": (
            ctypes.c_int,
            [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64), _P],
        ),
        "lg_workspace_bytes": (ctypes.c_int, [_P, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_forward": (ctypes.c_int, [_P, ctypes.POINTER(LGInputs), ctypes.POINTER(LGOutputs), _P, sz, _P]),
        "lg_filter_workspace_bytes": (ctypes.c_int, [i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_filter_matches": (ctypes.c_int, [_P, i32, i32, i32, ctypes.c_double, _P, _P, _P, _P, _P, sz, _P]),
        "lg_sinkhorn_workspace_bytes": (ctypes.c_int, [i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_log_optimal_transport": (ctypes.c_int, [_P, ctypes.c_float, i32, i32, i32, i32, _P, _P, sz, _P]),
        "lg_filter_matches_ragged": (ctypes.c_int, [_P, i32, i32, i32, ctypes.c_double, _P, _P, _P, _P, _P, _P, _P, sz, _P]),
        "lg_log_optimal_transport_ragged": (ctypes.c_int, [_P, ctypes.c_float, i32, i32, i32, _P, _P, i32, _P, _P, sz, _P]),
        "lg_sinkhorn_rerun_count": (ctypes.c_int64, []),
        "lg_sinkhorn_force_exact": (ctypes.c_int, [ctypes.c_int]),
        "sg_forward_ragged": (ctypes.c_int, [_P, ctypes.POINTER(SGInputs), _P, _P, ctypes.POINTER(SGOutputs), _P, sz, _P]),
        "lg_profile_enable": (ctypes.c_int, [_P, ctypes.c_int]),
        "lg_attention_workspace_bytes": (ctypes.c_int, [i32, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_attention": (
            ctypes.c_int,
            [_P, _P, _P, i32, i32, i32, i32, ctypes.c_float, i32, _P, _P, sz, _P],
        ),
        "lg_linear_workspace_bytes": (ctypes.c_int, [i32, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_linear": (ctypes.c_int, [ctypes.POINTER(LGLinearArgs), _P, sz, _P]),
        "lg_plane_roundtrip": (ctypes.c_int, [_P, i32, i32, i32, i32, _P, ctypes.POINTER(i32), _P]),
        "sp_conv_layer_workspace_bytes": (ctypes.c_int, [i32] * 7 + [ctypes.POINTER(sz)]),
        "sp_conv_layer_rows": (ctypes.c_int, [i32, i32, i32, i32, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(i32)]),
        "sp_conv_layer": (ctypes.c_int, [ctypes.POINTER(SPConvLayerArgs), _P, sz, _P]),
        "sp_head_scores": (ctypes.c_int, [_P, i32, i32, i32, i32, _P, _P]),
        "sp_head_normalize": (ctypes.c_int, [_P, i32, _P, _P]),
        "lg_assign_workspace_bytes": (ctypes.c_int, [i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_assign": (ctypes.c_int, [ctypes.POINTER(LGAssignArgs), _P, sz, _P]),
        "lg_assignment_workspace_bytes": (ctypes.c_int, [_P, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_assignment_head": (ctypes.c_int, [_P, i32, _P, _P, i32, i32, i32, _P, _P, _P, _P, _P, sz, _P]),
        "lg_gt_homography_workspace_bytes": (ctypes.c_int, [i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_gt_matches_from_homography": (
            ctypes.c_int,
            [_P, _P, _P, i32, i32, i32, ctypes.c_double, ctypes.c_double, _P, _P, _P, _P, _P, _P, _P, _P, _P, sz, _P],
        ),
        "lg_gt_depth_workspace_bytes": (ctypes.c_int, [i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_gt_matches_from_pose_depth": (
            ctypes.c_int,
            [_P, _P, _P, i32, i32, _P, i32, i32, _P, _P, i32, _P, _P, i32, i32, i32] + [ctypes.c_double] * 4
            + [_P] * 15 + [sz, _P],
        ),
        "lg_gt_line_thresholds": (
            ctypes.c_int, [i32, ctypes.c_double, ctypes.c_double, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "lg_gt_line_counts_workspace_bytes": (ctypes.c_int, [i32, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_gt_line_counts_homography": (
            ctypes.c_int,
            [_P, _P, _P] + [i32] * 8 + [ctypes.c_double, ctypes.c_double] + [_P] * 5 + [sz, _P],
        ),
        "lg_gt_line_labels_workspace_bytes": (ctypes.c_int, [i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_gt_line_labels": (ctypes.c_int, [_P] * 6 + [i32] * 4 + [ctypes.c_double] + [_P] * 4 + [sz, _P]),
        "lg_linear_sum_assignment_workspace_bytes": (ctypes.c_int, [i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_linear_sum_assignment": (ctypes.c_int, [_P, i32, i32, i32, _P, _P, _P, sz, _P]),
        "lg_gt_line_depth_thresholds": (
            ctypes.c_int,
            [i32, ctypes.c_double, ctypes.c_double, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "lg_gt_line_counts_pose_depth_workspace_bytes": (ctypes.c_int, [i32, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_gt_line_counts_pose_depth": (
            ctypes.c_int,
            [_P, _P, _P, i32, i32, _P, i32, i32] + [i32] * 4 + [_P, _P, i32, _P, _P] + [i32] * 4
            + [ctypes.c_double, ctypes.c_double] + [_P] * 9 + [sz, _P],
        ),
        "lg_gt_line_labels_visibility_workspace_bytes": (ctypes.c_int, [i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_gt_line_labels_visibility": (
            ctypes.c_int, [_P] * 10 + [i32] * 4 + [ctypes.c_double] + [_P] * 4 + [sz, _P]),
        "lg_nn_workspace_bytes": (ctypes.c_int, [i32, i32, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_nn_match": (
            ctypes.c_int,
            [_P, _P, i32, i32, i32, i32, ctypes.c_double, ctypes.c_double, i32] + [_P] * 9 + [sz, _P],
        ),
        "lg_eval_matches": (ctypes.c_int, [_P] * 4 + [i32] * 3 + [_P] * 7 + [i32] + [_P] * 5),
        "lg_ransac_lds_matches": (i32, []),
        "lg_ransac_homography": (
            ctypes.c_int,
            [_P] * 3 + [i32] * 3 + [_P] * 3 + [i32, ctypes.c_double, ctypes.c_uint64, ctypes.c_double] + [_P] * 8,
        ),
        "lg_ransac_lines_lds_capacity": (ctypes.c_int, [_P, _P]),
        "lg_ransac_homography_lines": (
            ctypes.c_int,
            [_P] * 3 + [i32] * 3 + [_P] * 5 + [i32] * 2 + [_P] * 3
            + [i32, ctypes.c_double, ctypes.c_uint64, ctypes.c_double] + [_P] * 10,
        ),
        "lg_ransac_relpose": (
            ctypes.c_int,
            [_P] * 3 + [i32] * 3 + [_P] * 5 + [i32, ctypes.c_double, ctypes.c_uint64] + [_P] * 8,
        ),
        "lg_essential_5pt": (ctypes.c_int, [_P, i32, _P, _P, _P]),
        "lg_train_saved_bytes": (ctypes.c_int, [_P, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_train_saved_bytes_ex": (ctypes.c_int, [_P, i32, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_train_scratch_bytes": (ctypes.c_int, [_P, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_train_forward": (ctypes.c_int, [_P, _P, ctypes.POINTER(LGInputs), _P, _P, _P, sz, _P]),
        "lg_train_backward": (ctypes.c_int, [_P, _P, ctypes.POINTER(LGInputs), _P, sz, _P, _P, _P, _P, _P, _P, sz, _P]),
        "lg_head_scratch_bytes": (ctypes.c_int, [_P, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_head_backward": (
            ctypes.c_int,
            [_P, _P, i32, _P, _P, i32, i32, i32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, sz, _P],
        ),
        "lg_head_backward_from_forward": (
            ctypes.c_int,
            [_P, _P, i32, _P, _P, i32, i32, i32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, sz, _P],
        ),
        "lg_head_forward": (ctypes.c_int, [_P, _P, i32, _P, _P, i32, i32, i32, _P, _P, _P, _P, _P, sz, _P]),
        "lg_head_nll_forward": (
            ctypes.c_int,
            [_P, _P, i32, _P, _P, i32, i32, i32, _P, _P, _P, i32, ctypes.c_float, _P, _P, _P, _P, _P, _P, sz, _P],
        ),
        "lg_head_nll_backward": (
            ctypes.c_int,
            [_P, _P, i32, _P, _P, i32, i32, i32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, i32, _P, sz, _P],
        ),
        "lg_train_gemm_workspace_bytes": (ctypes.c_int, [i32, i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_train_gemm": (
            ctypes.c_int,
            [_P, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
             i32, i32, i32, i32, ctypes.c_float, ctypes.c_float, _P, i32, i32, _P, sz, _P],
        ),
        "lg_train_gemm_ex": (
            ctypes.c_int,
            [_P, _P, _P, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
             i32, i32, i32, i32, ctypes.c_float, ctypes.c_float, _P, i32, i32,
             _P, ctypes.c_int64, i32, _P, ctypes.c_int64, i32, _P, ctypes.c_int64, _P, _P, sz, _P],
        ),
        "lg_train_attention": (ctypes.c_int, [_P, _P, _P, i32, i32, i32, i32, ctypes.c_float, _P, _P, _P]),
        "lg_train_attention_backward": (
            ctypes.c_int,
            [_P, _P, _P, _P, _P, _P, i32, i32, i32, i32, ctypes.c_float, _P, _P, _P, _P, _P],
        ),
        "sp_create": (ctypes.c_int, [ctypes.POINTER(SPConfig), ctypes.c_int, ctypes.POINTER(_P)]),
        "sp_open_create": (ctypes.c_int, [ctypes.POINTER(SPOpenConfig), ctypes.c_int, ctypes.POINTER(_P)]),
        "sp_destroy": (ctypes.c_int, [_P]),
        "sp_weight_count": (ctypes.c_int, [_P]),
        "sp_weight_name": (ctypes.c_char_p, [_P, ctypes.c_int]),
        "sp_weight_numel": (ctypes.c_int64, [_P, ctypes.c_int]),
        "sp_load_weights": (
            ctypes.c_int,
            [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64), _P],
        ),
        "sp_workspace_bytes": (ctypes.c_int, [_P, i32, i32, i32, i32, i32, ctypes.POINTER(sz)]),
        "sp_forward": (ctypes.c_int, [_P, ctypes.POINTER(SPInputs), ctypes.POINTER(SPOutputs), _P, sz, _P]),
        "sp_sample_descriptors": (ctypes.c_int, [_P, _P, _P, i32, i32, _P, _P, sz, _P]),
        "sp_aliked_create": (ctypes.c_int, [ctypes.POINTER(AlikedConfig), ctypes.c_int, ctypes.POINTER(_P)]),
        "sp_aliked_destroy": (ctypes.c_int, [_P]),
        "sp_aliked_weight_count": (ctypes.c_int, [_P]),
        "sp_aliked_weight_name": (ctypes.c_char_p, [_P, ctypes.c_int]),
        "sp_aliked_weight_numel": (ctypes.c_int64, [_P, ctypes.c_int]),
        "sp_aliked_load_weights": (
            ctypes.c_int,
            [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64), _P],
        ),
        "sp_aliked_workspace_bytes": (ctypes.c_int, [_P, i32, i32, i32, i32, ctypes.POINTER(sz)]),
        "sp_aliked_forward": (ctypes.c_int, [_P, ctypes.POINTER(AlikedInputs), ctypes.POINTER(AlikedOutputs), _P, sz, _P]),
        "sp_aliked_deform_conv": (ctypes.c_int, [_P, _P, _P, _P, i32, i32, i32, i32, i32, _P, _P, sz, _P]),
        "sp_aliked_set_profile": (ctypes.c_int, [_P, i32]),
        "sp_aliked_stage_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
        "sg_gluestick_create": (ctypes.c_int, [ctypes.POINTER(GSConfig), ctypes.c_int, ctypes.POINTER(_P)]),
        "sg_gluestick_destroy": (ctypes.c_int, [_P]),
        "sg_gluestick_weight_count": (ctypes.c_int, [_P]),
        "sg_gluestick_weight_name": (ctypes.c_char_p, [_P, ctypes.c_int]),
        "sg_gluestick_weight_numel": (ctypes.c_int64, [_P, ctypes.c_int]),
        "sg_gluestick_load_weights": (
            ctypes.c_int,
            [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64), _P],
        ),
        "sg_gluestick_workspace_bytes": (ctypes.c_int, [_P, i32, i32, i32, i32, i32, ctypes.POINTER(sz)]),
        "sg_gluestick_forward": (ctypes.c_int, [_P, ctypes.POINTER(GSInputs), ctypes.POINTER(GSOutputs), _P, sz, _P]),
        "sg_gluestick_line_update": (ctypes.c_int, [_P, i32, _P, _P, _P, i32, i32, i32, _P, _P]),
        "sg_gluestick_double_softmax": (ctypes.c_int, [_P, ctypes.c_float, i32, i32, i32, _P, _P]),
        "sg_gluestick_line_scores": (ctypes.c_int, [_P, _P, _P, _P, i32, i32, i32, i32, i32, _P, _P]),
        "lg_wireframe_workspace_bytes": (ctypes.c_int, [i32, i32, i32, ctypes.POINTER(sz)]),
        "lg_wireframe_forward": (
            ctypes.c_int,
            [ctypes.POINTER(WFConfig), ctypes.POINTER(WFInputs), ctypes.POINTER(WFOutputs), _P, sz, _P],
        ),
        "lg_wireframe_connectivity": (ctypes.c_int, [_P, i32, i32, i32, i32, _P, _P]),
        "lg_sample_descriptors_corner": (ctypes.c_int, [_P, _P, i32, i32, i32, i32, i32, i32, _P, _P]),
        "sg_create": (ctypes.c_int, [ctypes.POINTER(SGConfig), ctypes.c_int, ctypes.POINTER(_P)]),
        "sg_destroy": (ctypes.c_int, [_P]),
        "sg_weight_count": (ctypes.c_int, [_P]),
        "sg_weight_name": (ctypes.c_char_p, [_P, ctypes.c_int]),
        "sg_weight_numel": (ctypes.c_int64, [_P, ctypes.c_int]),
        "sg_load_weights": (
            ctypes.c_int,
            [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int64), _P],
        ),
        "sg_workspace_bytes": (ctypes.c_int, [_P, i32, i32, i32, ctypes.POINTER(sz)]),
        "sg_forward": (ctypes.c_int, [_P, ctypes.POINTER(SGInputs), ctypes.POINTER(SGOutputs), _P, sz, _P]),
        "sg_nll_loss": (ctypes.c_int, [_P, i32, i32, i32, _P, _P, _P, i32, ctypes.c_float, _P, _P]),
        "sg_nll_workspace_bytes": (ctypes.c_int, [i32, i32, ctypes.POINTER(ctypes.c_size_t)]),
        "sg_nll_loss_ws": (ctypes.c_int, [_P, i32, i32, i32, _P, _P, _P, i32, ctypes.c_float, _P, _P, ctypes.c_size_t, _P]),
        # callbacks as void* (fnptr): NULL unregisters
        "lg_set_grad_ready_hook": (ctypes.c_int, [_P, _P, _P]),
        "sg_collective_floats": (sz, []),
        "sg_set_collective": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int64]),
        "sg_set_grad_ready_hook": (ctypes.c_int, [_P, _P, _P]),
        "sg_train_saved_bytes": (ctypes.c_int, [_P, i32, i32, i32, ctypes.POINTER(sz)]),
        "sg_train_saved_tensor": (ctypes.c_int, [_P, i32, i32, i32, ctypes.c_char_p, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
        "sg_train_scratch_bytes": (ctypes.c_int, [_P, i32, i32, i32, ctypes.POINTER(sz)]),
        "sg_train_forward": (ctypes.c_int, [_P, _P, ctypes.POINTER(SGInputs), ctypes.POINTER(SGOutputs), _P, sz, _P]),
        "sg_train_backward": (ctypes.c_int, [_P, _P, ctypes.POINTER(SGInputs), _P, sz, _P, _P, _P, _P, _P, _P, sz, _P]),
        "sg_nll_backward": (ctypes.c_int, [_P, _P, _P, _P, i32, i32, i32, _P, _P, _P, i32, ctypes.c_float, _P, _P]),
        "lg_profile_read": (
            ctypes.c_int,
            [_P, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64),
             ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)],
        ),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.lg_abi_version() != ABI_VERSION:
        raise LightGlueLibError(f"ABI mismatch: library {lib.lg_abi_version()} != binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc, what):
    if rc != LG_OK:
        msg = load().lg_last_error().decode(errors="replace")
        if rc == LG_E_INVALID and msg.startswith("max():"):
            raise IndexError(msg)  # same exception type as the reference's torch.max on an empty dim
        raise LightGlueLibError(f"{what} failed ({rc}): {msg}")
