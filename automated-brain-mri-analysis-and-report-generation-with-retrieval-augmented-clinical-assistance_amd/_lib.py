"""ctypes binding of include/mi355_nnunet.h.

There is no Python/CPU fallback: if the shared library is missing the import of any compute
entry point raises, and on a machine without a gfx950 device the library itself returns
MI355_ERR_NO_DEVICE.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

from . import _build

c_float_p = C.POINTER(C.c_float)
c_int32_p = C.POINTER(C.c_int32)

NORM_NONE, NORM_BATCH, NORM_INSTANCE, NORM_GROUP = 0, 1, 2, 3
F32, F16 = 0, 1
NONLIN_IDENTITY, NONLIN_SIGMOID, NONLIN_SOFTMAX = 0, 1, 2

#: every symbol include/mi355_nnunet.h declares (tests check that the .so exports all of them)
EXPORTS = [
    "mi355_last_error", "mi355_version", "mi355_device_count", "mi355_unet_create", "mi355_unet_destroy",
    "mi355_unet_flops", "mi355_unet_forward", "mi355_sw_predict", "mi355_compute_steps", "mi355_sw_partial",
    "mi355_sw_finish", "mi355_regions_to_labels", "mi355_label_ensemble", "mi355_prob_mean",
    "mi355_zscore_masked", "mi355_conv3d_ndhwc", "mi355_tconv3d_ndhwc", "mi355_profile_enable",
    "mi355_profile_read", "mi355_conv3d_ndhwc_f16", "mi355_tconv3d_ndhwc_f16",
    "mi355_label_remap", "mi355_label_confusion", "mi355_cosine_topk", "mi355_crop_mask", "mi355_label_stats",
    "mi355_last_conv_kernel",
    "mi355_conv3d_sums_ndhwc", "mi355_conv3d_fused_ndhwc", "mi355_conv3d_plan", "mi355_conv_kernel_names",
    "mi355_sw_partial_folds", "mi355_sw_finish_folds",
    "mi355_resize_axis", "mi355_clip_to_range_of", "mi355_threshold_ge", "mi355_mask_to_float",
    "mi355_label_components", "mi355_component_stats", "mi355_component_filter",
    "mi355_binary_morphology", "mi355_edt_squared", "mi355_surface_gradient_stats", "mi355_mask_second_moments",
    "mi355_masked_moments", "mi355_flag_from_labels", "mi355_flag_from_flags",
    "mi355_masked_percentiles", "mi355_masked_percentiles_multi",
    "mi355_binary_fill_holes", "mi355_sobel_magnitude_stats", "mi355_radial_shell_moments", "mi355_face_slab_counts",
    "mi355_axis_counts", "mi355_box_counts", "mi355_select_ranked", "mi355_min_pair_dist2", "mi355_masked_min_i32",
    "mi355_label_components_nb", "mi355_cityblock_distance", "mi355_flag_from_i32", "mi355_flag_from_box", "mi355_masked_order_stats_i32",
    "mi355_column_count_max",
    "mi355_region_surfaces", "mi355_edt_to_flagged_f64", "mi355_gather_flagged_f64",
    "mi355_binary_morphology_nb", "mi355_label_pair_counts", "mi355_label_lookup", "mi355_label_lookup_i32",
    "mi355_stage0_plan", "mi355_skip_share_plan", "mi355_conv3d_wino3_ndhwc",
    "mi355_norm_finalize", "mi355_norm_apply", "mi355_extract_tiles", "mi355_head_logits", "mi355_head_aggregate",
    "mi355_logits_aggregate", "mi355_cnt_add_tile", "mi355_stage0_gather", "mi355_stage0_mask",
    "mi355_stage0_view_plan", "mi355_conv3d_s2dma_view_ndhwc", "mi355_conv3d_wino3_view_ndhwc", "mi355_stage0_gather_shells",
    "mi355_logits_aggregate_tiles", "mi355_stage0_merge_plan", "mi355_stage0_gather_merged",
    "mi355_scratch_sizes", "mi355_scratch_fill", "mi355_scratch_release", "mi355_scratch_zero_pages",
    "mi355_level1_share_plan",
    "mi355_reverse_axes",
    "mi355_conv3d_plan_hinted", "mi355_conv3d_s2dma_hinted_ndhwc", "mi355_stage0_gather_boxes",
    "mi355_sw_partial_folds_moments", "mi355_sw_finish_moments", "mi355_logits_aggregate_m2", "mi355_logits_aggregate_tiles_m2",
    "mi355_head_aggregate_m2", "mi355_uncertainty_maps", "mi355_uncertainty_stats",
    "mi355_live_allocations",
    "mi355_tconv3d_plan",
    "mi355_conv_s2_split_pack", "mi355_conv3d_s2dma_concat_ndhwc",
]


class ConvDesc(C.Structure):
    _fields_ = [("cin", C.c_int32), ("cout", C.c_int32), ("stride", C.c_int32),
                ("weight", c_float_p), ("bias", c_float_p), ("gamma", c_float_p), ("beta", c_float_p),
                ("running_mean", c_float_p), ("running_var", c_float_p)]


class TConvDesc(C.Structure):
    _fields_ = [("cin", C.c_int32), ("cout", C.c_int32), ("weight", c_float_p)]


class HeadDesc(C.Structure):
    _fields_ = [("cin", C.c_int32), ("num_classes", C.c_int32), ("weight", c_float_p), ("bias", c_float_p)]


class UNetDesc(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("num_classes", C.c_int32), ("num_pool", C.c_int32),
                ("norm", C.c_int32), ("num_groups", C.c_int32), ("eps", C.c_float), ("lrelu_slope", C.c_float),
                ("nonlin_first", C.c_int32), ("dtype", C.c_int32),
                ("enc_convs", c_int32_p), ("dec_convs", c_int32_p),
                ("convs", C.POINTER(ConvDesc)), ("n_convs", C.c_int32),
                ("tconvs", C.POINTER(TConvDesc)), ("head", HeadDesc)]


class SwOpts(C.Structure):
    _fields_ = [("patch", C.c_int32 * 3), ("step_size", C.c_double), ("use_gaussian", C.c_int32),
                ("mirror_axes", C.c_int32), ("nonlin", C.c_int32), ("batch_tiles", C.c_int32)]


class ProfEntry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


class ConvPlan(C.Structure):
    _fields_ = [("rc", C.c_int32), ("kernel", C.c_char * 96), ("grid", C.c_int32 * 3), ("lds_bytes", C.c_int64),
                ("splitk", C.c_int32), ("tile", C.c_int32 * 3), ("fuses_in_norm", C.c_int32)]


class Stage0Geom(C.Structure):
    _fields_ = [("shared", C.c_int32), ("r", C.c_int32), ("n_tiles", C.c_int32), ("n_mirrors", C.c_int32),
                ("padded", C.c_int32 * 3), ("volume", C.c_int32 * 3), ("slab_thickness", C.c_int32 * 3)]


class SkipShareNet(C.Structure):
    _fields_ = [("dtype", C.c_int32), ("norm", C.c_int32), ("nonlin_first", C.c_int32), ("enc0_blocks", C.c_int32),
                ("stride", C.c_int32), ("skip_is_enc0", C.c_int32), ("c_up", C.c_int32), ("c_skip", C.c_int32), ("cout", C.c_int32),
                ("head_ncls", C.c_int32)]


class SkipShareGeom(C.Structure):
    _fields_ = [("stage0_shared", C.c_int32), ("skip_shared", C.c_int32), ("r", C.c_int32), ("skip_shell", C.c_int32),
                ("n_tiles", C.c_int32), ("n_mirrors", C.c_int32), ("volume", C.c_int32 * 3), ("slab_thickness", C.c_int32 * 3)]


class Stage0Sample(C.Structure):
    _fields_ = [("tile", C.c_int32), ("mirror", C.c_int32), ("origin", C.c_int32 * 3), ("face", C.c_int32 * 6),
                ("slab_origin", (C.c_int32 * 3) * 6), ("slab_shape", (C.c_int32 * 3) * 6)]


class Stage0GatherSample(C.Structure):
    _fields_ = [("wv", C.c_int32), ("origin", C.c_int32 * 3), ("slab", C.c_int32 * 6)]


class Stage0GatherArgs(C.Structure):
    _fields_ = [("wv_dev", C.c_void_p), ("slab_dev", C.c_void_p * 3), ("out_dev", C.c_void_p),
                ("patch", C.c_int32 * 3), ("volume", C.c_int32 * 3), ("slab_thickness", C.c_int32 * 3),
                ("r", C.c_int32), ("channels", C.c_int32), ("n_samples", C.c_int32), ("samples", Stage0GatherSample * 64)]


class Stage0MergeGeom(C.Structure):
    _fields_ = [("shared", C.c_int32), ("r", C.c_int32), ("rs", C.c_int32), ("n_tiles", C.c_int32), ("n_mirrors", C.c_int32),
                ("padded", C.c_int32 * 3), ("volume", C.c_int32 * 3), ("slab_thickness", C.c_int32 * 3), ("n_slabs", C.c_int32 * 3),
                ("slab_shape", (C.c_int32 * 3) * 3), ("voxels", C.c_int64 * 3), ("voxels_per_tile", C.c_int64)]


class Stage0MergeSlab(C.Structure):
    _fields_ = [("axis", C.c_int32), ("mirror", C.c_int32), ("side", C.c_int32), ("origin", C.c_int32 * 3)]


class Stage0MergeSample(C.Structure):
    _fields_ = [("tile", C.c_int32), ("mirror", C.c_int32), ("origin", C.c_int32 * 3), ("slab", C.c_int32 * 6),
                ("offset", (C.c_int32 * 3) * 6)]


class Stage0GatherMergedArgs(C.Structure):
    _fields_ = [("base", Stage0GatherArgs), ("slab_shape", (C.c_int32 * 3) * 3), ("spans_volume", (C.c_int32 * 3) * 3),
                ("wv2_dev", C.c_void_p), ("slab2_dev", C.c_void_p * 3), ("out2_dev", C.c_void_p), ("r2", C.c_int32), ("channels2", C.c_int32)]


class Stage0GatherBoxesArgs(C.Structure):
    _fields_ = [("merged", Stage0GatherMergedArgs), ("tile", C.c_int32 * 3), ("sub", (C.c_int32 * 3) * 64)]


class Stage0ViewGeom(C.Structure):
    _fields_ = [("enc0_viewed", C.c_int32), ("half_viewed", C.c_int32), ("depth", C.c_int32 * 2), ("n_tiles", C.c_int32),
                ("n_mirrors", C.c_int32), ("volume", C.c_int32 * 3)]


class Stage0ViewSample(C.Structure):
    _fields_ = [("offset", C.c_int64), ("faces", C.c_int32), ("pad_", C.c_int32), ("shell_voxels", C.c_int64 * 2)]


class Stage0ViewItem(C.Structure):
    _fields_ = [("wv", C.c_int32), ("origin", C.c_int32 * 3), ("faces", C.c_int32)]


class Stage0View(C.Structure):
    _fields_ = [("src_dev", C.c_void_p), ("n_wv", C.c_int32), ("volume", C.c_int32 * 3), ("depth", C.c_int32), ("n_samples", C.c_int32),
                ("samples", Stage0ViewItem * 64)]


class Level1ShareNet(C.Structure):
    _fields_ = [("last", SkipShareNet), ("num_pool", C.c_int32), ("enc1_blocks", C.c_int32), ("c_level1", C.c_int32),
                ("skip_is_enc1", C.c_int32), ("dec1_blocks", C.c_int32), ("c_up1", C.c_int32), ("cout1", C.c_int32)]


class Level1ShareGeom(C.Structure):
    _fields_ = [("possible", C.c_int32), ("on", C.c_int32), ("r0", C.c_int32), ("k1", C.c_int32), ("d1", C.c_int32), ("dS", C.c_int32),
                ("n_tiles", C.c_int32), ("n_mirrors", C.c_int32), ("n_regions", C.c_int32), ("padded", C.c_int32 * 3),
                ("volume", C.c_int32 * 3), ("stage0_slab_thickness", C.c_int32 * 3), ("merged", C.c_int32 * 3), ("region", C.c_int32 * 3),
                ("slab_thickness", C.c_int32 * 3), ("n_slabs", C.c_int32 * 3),
                ("region_voxels", C.c_int64), ("slab_voxels", C.c_int64), ("tile_voxels", C.c_int64)]


class Level1ShareRegion(C.Structure):
    _fields_ = [("mirror", C.c_int32), ("origin", C.c_int32 * 3), ("faces", C.c_int32)]


class Level1ShareSample(C.Structure):
    _fields_ = [("tile", C.c_int32), ("mirror", C.c_int32), ("region", C.c_int32), ("origin", C.c_int32 * 3), ("origin1", C.c_int32 * 3),
                ("faces", C.c_int32), ("slab", C.c_int32 * 6), ("slab_offset", (C.c_int32 * 3) * 6), ("slab_shape", (C.c_int32 * 3) * 6)]


class Mi355Error(RuntimeError):
    pass


_lib = None


def lib_path() -> Path:
    return _build.LIB_PATH


def load():
    """Load (once) the HIP library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not path.exists():
        raise Mi355Error(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    if _build.needs_build():
        # the digest of csrc/ differs from the one the library was built from: rebuild (under the build lock) rather than run stale code
        try:
            _build.build()
        except Exception as e:  # no hipcc on this machine: say so instead of silently running the old library
            import warnings
            warnings.warn(f"{path} was built from a different csrc/ and could not be rebuilt ({e}); running the stale library")
    # torch first: its wheel bundles a HIP runtime of its own (torch/lib/libamdhip64.so), and the library must share THAT runtime -
    # it is handed torch's device pointers and streams.  Loaded before torch, this library pulls in /opt/rocm's libamdhip64 under
    # the same SONAME and the process ends up with one runtime torch was not built against (seen in round 5: build() + smoke() in
    # one process - mi355_device_count() = 0 on a box with a GPU).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(str(path))
    vp = C.c_void_p
    lib.mi355_last_error.restype = C.c_char_p
    lib.mi355_last_conv_kernel.restype = C.c_char_p
    lib.mi355_unet_create.argtypes = [C.POINTER(UNetDesc), C.POINTER(vp)]
    lib.mi355_unet_destroy.argtypes = [vp]
    lib.mi355_unet_flops.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.mi355_unet_flops.restype = C.c_int64
    lib.mi355_unet_forward.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.mi355_sw_predict.argtypes = [C.POINTER(vp), C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(SwOpts), vp, vp]
    lib.mi355_compute_steps.argtypes = [C.c_int, C.c_int, C.c_double, c_int32_p, C.c_int]
    lib.mi355_sw_partial.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(SwOpts), C.c_int, C.c_int, vp, vp, vp]
    lib.mi355_sw_finish.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, c_int32_p, vp, vp]
    lib.mi355_sw_partial_folds.argtypes = [C.POINTER(vp), C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(SwOpts), C.c_int, C.c_int, vp, vp, vp]
    lib.mi355_sw_finish_folds.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, c_int32_p, C.c_int, vp, vp]
    lib.mi355_regions_to_labels.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, c_int32_p, c_int32_p, c_int32_p, vp, vp]
    lib.mi355_label_ensemble.argtypes = [vp, vp, vp, C.c_int64, vp]
    lib.mi355_prob_mean.argtypes = [vp, vp, vp, C.c_int64, vp]
    lib.mi355_zscore_masked.argtypes = [vp, vp, C.c_int, C.c_int64, vp]
    lib.mi355_conv3d_ndhwc.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int,
                                       C.c_int, C.c_int, C.c_float, C.c_int, vp, vp]
    lib.mi355_tconv3d_ndhwc.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_int, vp, vp]
    lib.mi355_conv3d_ndhwc_f16.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int,
                                           C.c_int, C.c_int, C.c_float, vp, vp]
    lib.mi355_tconv3d_ndhwc_f16.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_int, vp, vp]
    lib.mi355_conv3d_sums_ndhwc.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int,
                                            C.c_int, C.c_int, C.c_float, vp, vp, vp]
    lib.mi355_conv3d_fused_ndhwc.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p,
                                             c_float_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, C.c_int, vp, vp,
                                             C.c_int, vp, vp, vp, vp]
    lib.mi355_conv3d_plan.argtypes = [C.c_int] * 13 + [C.POINTER(ConvPlan)]
    lib.mi355_conv3d_plan_hinted.argtypes = [C.c_int] * 14 + [C.POINTER(ConvPlan)]
    lib.mi355_tconv3d_plan.argtypes = [C.c_int] * 7 + [C.POINTER(ConvPlan)]
    lib.mi355_conv_kernel_names.argtypes = [C.c_char_p, C.c_int64]
    lib.mi355_conv_kernel_names.restype = C.c_int64
    lib.mi355_stage0_plan.argtypes = [C.c_int, C.c_int, C.c_int, c_int32_p, C.c_double, C.c_int, C.c_int, C.POINTER(Stage0Geom),
                                      C.POINTER(Stage0Sample), C.c_int]
    lib.mi355_skip_share_plan.argtypes = [C.c_int, C.c_int, C.c_int, c_int32_p, C.c_double, C.c_int, C.POINTER(SkipShareNet), C.c_int,
                                          C.c_int, C.c_int, C.POINTER(SkipShareGeom)]
    lib.mi355_conv3d_wino3_ndhwc.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p,
                                             C.c_int, C.c_int, C.c_float, vp, vp, vp]
    lib.mi355_label_remap.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_uint8), vp]
    lib.mi355_label_confusion.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(C.c_uint64), vp]
    lib.mi355_cosine_topk.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, c_int32_p, c_float_p, vp]
    lib.mi355_crop_mask.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, c_int32_p, vp]
    lib.mi355_label_stats.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), vp]
    lib.mi355_resize_axis.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int, vp]
    lib.mi355_clip_to_range_of.argtypes = [vp, C.c_int64, C.c_int64, vp, C.c_int64, vp]
    lib.mi355_threshold_ge.argtypes = [vp, C.c_float, vp, C.c_int64, vp]
    lib.mi355_mask_to_float.argtypes = [vp, vp, C.c_int64, vp]
    lib.mi355_label_components.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, c_int32_p, vp]
    lib.mi355_component_stats.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), vp]
    lib.mi355_component_filter.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_uint8), C.c_int, vp, vp]
    lib.mi355_binary_morphology.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.mi355_edt_squared.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.mi355_surface_gradient_stats.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), vp]
    lib.mi355_mask_second_moments.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), vp]
    lib.mi355_masked_moments.argtypes = [vp, C.c_int, vp, C.c_int64, C.POINTER(C.c_double), vp]
    lib.mi355_flag_from_labels.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int, vp, C.c_int64, vp]
    lib.mi355_flag_from_flags.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_double, C.c_double, C.c_int64, vp]
    lib.mi355_masked_percentiles.argtypes = [vp, C.c_int64, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.c_int,
                                             C.POINTER(C.c_int64), c_float_p, c_float_p, vp]
    lib.mi355_masked_percentiles_multi.argtypes = [C.POINTER(vp), C.c_int, C.c_int64, vp, c_int32_p, c_int32_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                   C.POINTER(C.POINTER(C.c_double)), c_int32_p, C.POINTER(C.c_int64), c_float_p, c_float_p, c_int32_p, vp]
    lib.mi355_binary_fill_holes.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_int64), vp]
    lib.mi355_sobel_magnitude_stats.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), vp]
    lib.mi355_radial_shell_moments.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double, C.c_double,
                                               C.POINTER(C.c_double), vp]
    lib.mi355_face_slab_counts.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), vp]
    lib.mi355_axis_counts.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), vp]
    lib.mi355_box_counts.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_int32_p, C.c_int, C.POINTER(C.c_int64), vp]
    lib.mi355_select_ranked.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.c_int, vp, C.POINTER(C.c_int64), vp]
    lib.mi355_min_pair_dist2.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), vp]
    lib.mi355_masked_min_i32.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int64, c_int32_p, C.POINTER(C.c_int64), vp]
    lib.mi355_label_components_nb.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, c_int32_p, vp]
    lib.mi355_cityblock_distance.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    lib.mi355_flag_from_i32.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int32, C.c_int32, C.c_int64, vp]
    lib.mi355_flag_from_box.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_int32_p, vp]
    lib.mi355_masked_order_stats_i32.argtypes = [vp, C.c_int64, vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int64), c_int32_p,
                                                 c_int32_p, vp]
    lib.mi355_column_count_max.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), vp]
    lib.mi355_region_surfaces.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), vp, C.c_int64, vp]
    lib.mi355_edt_to_flagged_f64.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_int32_p, c_int32_p, C.c_int, C.POINTER(C.c_double), vp, C.c_int64, vp, vp]
    lib.mi355_gather_flagged_f64.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, c_int32_p, c_int32_p, C.c_int, vp, C.c_int64, vp, C.c_int64,
                                             C.POINTER(C.c_int64), vp]
    lib.mi355_binary_morphology_nb.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int64, vp]
    lib.mi355_label_pair_counts.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int64), vp]
    lib.mi355_label_lookup.argtypes = [vp, C.c_int64, C.c_int, C.POINTER(C.c_uint8), vp, C.c_int64, vp, vp]
    lib.mi355_label_lookup_i32.argtypes = [vp, C.c_int64, C.c_int, c_int32_p, vp, C.c_int64, vp, vp]
    lib.mi355_reverse_axes.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    lib.mi355_norm_finalize.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_float, vp, vp, vp, vp, vp]
    lib.mi355_norm_apply.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.c_int, vp, vp, C.c_int, C.c_float, vp]
    lib.mi355_extract_tiles.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, c_int32_p, c_int32_p, C.c_int, c_int32_p, C.c_int, vp,
                                        C.c_int, vp]
    lib.mi355_head_logits.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.c_int, c_float_p, c_float_p, C.c_int, vp, vp, C.c_float, vp, vp]
    lib.mi355_head_aggregate.argtypes = [vp, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int, vp, vp, C.c_float, C.c_int, c_int32_p,
                                         C.c_int, c_int32_p, C.c_int, vp, vp, vp, c_int32_p, c_int32_p, vp]
    lib.mi355_logits_aggregate.argtypes = [vp, C.c_int, C.c_int, c_int32_p, C.c_int, c_int32_p, C.c_int, vp, vp, vp, c_int32_p,
                                           c_int32_p, vp]
    lib.mi355_logits_aggregate_tiles.argtypes = [vp, C.c_int, C.c_int, c_int32_p, C.c_int, c_int32_p, C.c_int, vp, vp, vp, c_int32_p,
                                                 c_int32_p, C.c_int, vp]
    lib.mi355_head_aggregate_m2.argtypes = [vp, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int, vp, vp, C.c_float, C.c_int, c_int32_p,
                                            C.c_int, c_int32_p, C.c_int, vp, vp, vp, vp, c_int32_p, c_int32_p, vp]
    lib.mi355_logits_aggregate_m2.argtypes = [vp, C.c_int, C.c_int, c_int32_p, C.c_int, c_int32_p, C.c_int, vp, vp, vp, vp, c_int32_p,
                                              c_int32_p, vp]
    lib.mi355_logits_aggregate_tiles_m2.argtypes = [vp, C.c_int, C.c_int, c_int32_p, C.c_int, c_int32_p, C.c_int, vp, vp, vp, vp, c_int32_p,
                                                    c_int32_p, C.c_int, vp]
    lib.mi355_sw_partial_folds_moments.argtypes = [C.POINTER(vp), C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(SwOpts), C.c_int, C.c_int,
                                                   vp, vp, vp, vp]
    lib.mi355_sw_finish_moments.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, c_int32_p, C.c_int, vp, vp, vp]
    lib.mi355_uncertainty_maps.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, c_int32_p, c_int32_p, vp, vp, vp]
    lib.mi355_uncertainty_stats.argtypes = [vp, vp, vp, C.c_int, C.c_int64, c_float_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_double), vp]
    lib.mi355_cnt_add_tile.argtypes = [vp, c_int32_p, vp, c_int32_p, c_int32_p, vp]
    lib.mi355_stage0_gather.argtypes = [C.POINTER(Stage0GatherArgs), vp]
    lib.mi355_stage0_mask.argtypes = [vp, C.c_int, c_int32_p, c_int32_p, C.c_int, vp]
    lib.mi355_stage0_merge_plan.argtypes = [C.c_int, C.c_int, C.c_int, c_int32_p, C.c_double, C.c_int, C.c_int, C.c_int, C.POINTER(Stage0MergeGeom),
                                            C.POINTER(Stage0MergeSlab), C.c_int, C.POINTER(Stage0MergeSample), C.c_int]
    lib.mi355_stage0_gather_merged.argtypes = [C.POINTER(Stage0GatherMergedArgs), C.c_int, vp]
    lib.mi355_stage0_gather_shells.argtypes = [C.POINTER(Stage0GatherArgs), vp]
    lib.mi355_stage0_gather_boxes.argtypes = [C.POINTER(Stage0GatherBoxesArgs), C.c_int, C.c_int, vp]
    lib.mi355_stage0_view_plan.argtypes = [C.c_int, C.c_int, C.c_int, c_int32_p, C.c_double, C.c_int, C.POINTER(SkipShareNet), C.c_int, C.c_int,
                                           C.POINTER(Stage0ViewGeom), C.POINTER(Stage0ViewSample), C.c_int]
    lib.mi355_conv3d_s2dma_view_ndhwc.argtypes = [vp, C.POINTER(Stage0View), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p,
                                                  C.c_int, C.c_int, C.c_float, C.c_int, vp, vp]
    lib.mi355_conv3d_s2dma_hinted_ndhwc.argtypes = [vp, C.POINTER(Stage0View), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p,
                                                    C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, vp, vp]
    lib.mi355_conv3d_s2dma_concat_ndhwc.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p,
                                                    C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, vp, vp]
    lib.mi355_conv_s2_split_pack.argtypes = [c_float_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint16), C.c_int64]
    lib.mi355_conv_s2_split_pack.restype = C.c_int64
    lib.mi355_conv3d_wino3_view_ndhwc.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int, C.c_int,
                                                  C.c_float, vp, C.POINTER(Stage0View), vp, vp]
    lib.mi355_level1_share_plan.argtypes = [C.c_int, C.c_int, C.c_int, c_int32_p, C.c_double, C.c_int, C.POINTER(Level1ShareNet), C.c_int,
                                            C.POINTER(Level1ShareGeom), C.POINTER(Level1ShareRegion), C.c_int, C.POINTER(Level1ShareSample), C.c_int]
    lib.mi355_scratch_sizes.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
    lib.mi355_scratch_fill.argtypes = [vp, C.c_int, C.c_uint32]
    lib.mi355_scratch_fill.restype = C.c_int64
    lib.mi355_scratch_release.argtypes = [vp]
    lib.mi355_scratch_zero_pages.argtypes = [C.POINTER(C.c_int64)]
    lib.mi355_live_allocations.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.mi355_profile_enable.argtypes = [vp, C.c_int]
    lib.mi355_profile_read.argtypes = [vp, C.POINTER(ProfEntry), C.c_int]
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc < 0:
        msg = load().mi355_last_error()
        raise Mi355Error(f"{what or 'mi355 call'} failed ({rc}): {msg.decode() if msg else '?'}")


def fptr(a):
    """float32 C-contiguous numpy array -> float* (None -> NULL)."""
    if a is None:
        return None
    return a.ctypes.data_as(c_float_p)
