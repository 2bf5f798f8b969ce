/*
 * mi355_nnunet.h - C ABI of the MI355X-native nnU-Net (BraTS) sliding-window predictor.
 *
 * This is the drop-in boundary for the one hot path of the reference
 * (SURVEY.md section 8b).  The reference is pure Python; what a maintainer would bind
 * is a ctypes stub (INTEGRATION.md shows it).  Each entry point names the reference
 * interface it replaces (paths relative to the reference repo):
 *
 *   mi355_unet_create        model_architecture/generic_UNet.py:188-421  Generic_UNet.__init__
 *                            + nnunet load_model_and_checkpoint_files / trainer.load_checkpoint_ram
 *                              as called at run_brats2021_inference_singlethread.py:178-183,95,113
 *   mi355_unet_forward       model_architecture/generic_UNet.py:423-446  Generic_UNet.forward
 *   mi355_sw_predict         trainer.predict_preprocessed_data_return_seg_and_softmax(...)[1]
 *                            called at run_brats2021_inference_singlethread.py:97-106,114-123
 *                            (+ the fold mean at :128 when several handles are given)
 *   mi355_regions_to_labels  save_segmentation_nifti_from_softmax(..., region_class_order=(1,2,3))
 *                            called at run_brats2021_inference_singlethread.py:144-156
 *   mi355_label_ensemble     run_brats2021_inference_singlethread.py:299-305  np.round((s1+s2)/2)
 *   mi355_prob_mean          archived/kaist_original_inference.py:30-32 (nnUNet_ensemble: mean of two softmax volumes)
 *   mi355_zscore_masked      trainer.preprocess_patient -> nonCT + use_mask_for_norm normalisation,
 *                            called at run_brats2021_inference_singlethread.py:89
 *   mi355_resize_axis        trainer.preprocess_patient -> resample_patient (same call) and the resampling inside
 *                            save_segmentation_nifti_from_softmax (:131-138, :144-156)
 *
 * Conventions: every function returns 0 on success and a negative code on failure;
 * mi355_last_error() gives the message of the calling thread's last failure.
 * All "dev" pointers are device (HBM) pointers on the current HIP device; the caller
 * owns them.  The library owns its weights and activation arena.  `stream` is a
 * hipStream_t passed as void* (NULL = default stream).  ONE PROCESS PER GPU: the library binds
 * to the HIP device that is current at its first compute call (weights, arena and scratch
 * buffers live there) and every later call fails with MI355_ERR_INVALID while another device
 * is current.  The activation arena and every scratch buffer exist once per STREAM ("lane", round 5): work
 * issued on one stream is ordered by that stream and shares its arena across handles; up to four streams may
 * carry work at the same time (a fifth takes over the least recently used lane after a device synchronise).
 * A handle may be used on two streams at once (its weights are read-only); not from two threads while its
 * profiling log is enabled.  There is NO CPU fallback: on a
 * machine without a gfx950 device every compute entry point fails with MI355_ERR_NO_DEVICE.
 */
#ifndef MI355_NNUNET_H
#define MI355_NNUNET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_OK 0
#define MI355_ERR_INVALID (-1)
#define MI355_ERR_HIP (-2)
#define MI355_ERR_NO_DEVICE (-3)
#define MI355_ERR_UNSUPPORTED (-4)

enum { MI355_NORM_NONE = 0, MI355_NORM_BATCH = 1, MI355_NORM_INSTANCE = 2, MI355_NORM_GROUP = 3 };
enum { MI355_F32 = 0, MI355_F16 = 1 };
enum { MI355_NONLIN_IDENTITY = 0, MI355_NONLIN_SIGMOID = 1, MI355_NONLIN_SOFTMAX = 2 };

/* One ConvDropoutNormNonlin block (generic_UNet.py:27-72): Conv3d k=3 p=1 + norm + LeakyReLU.
 * All pointers are HOST pointers to fp32 data in the PyTorch layouts; they are read
 * during mi355_unet_create only. */
typedef struct {
    int32_t cin, cout, stride;
    const float *weight;       /* [cout][cin][3][3][3] */
    const float *bias;         /* [cout] or NULL */
    const float *gamma, *beta; /* norm affine [cout]; NULL -> 1 / 0 */
    const float *running_mean, *running_var; /* MI355_NORM_BATCH only */
} mi355_conv_desc;

/* ConvTranspose3d k=2 s=2 bias=False (generic_UNet.py:363-364). */
typedef struct {
    int32_t cin, cout;
    const float *weight; /* [cin][cout][2][2][2] */
} mi355_tconv_desc;

/* seg_outputs[-1]: Conv3d 1x1x1 (generic_UNet.py:389-391). */
typedef struct {
    int32_t cin, num_classes;
    const float *weight; /* [num_classes][cin] */
    const float *bias;   /* [num_classes] or NULL (seg_output_use_bias=False) */
} mi355_head_desc;

typedef struct {
    int32_t in_channels, num_classes, num_pool;
    int32_t norm;       /* MI355_NORM_* ; BATCH is eval mode and is folded into the conv */
    int32_t num_groups; /* MI355_NORM_GROUP */
    float eps, lrelu_slope;
    int32_t nonlin_first; /* 1 = ConvDropoutNonlinNorm (generic_UNet.py:75-80) */
    int32_t dtype;        /* MI355_F32 | MI355_F16 (storage; accumulation is always fp32) */
    const int32_t *enc_convs; /* [num_pool+1] convs per encoder stage; last = bottleneck */
    const int32_t *dec_convs; /* [num_pool]   convs per decoder stage */
    const mi355_conv_desc *convs; /* execution order: encoder stages, bottleneck, decoder stages */
    int32_t n_convs;
    const mi355_tconv_desc *tconvs; /* [num_pool] */
    mi355_head_desc head;
} mi355_unet_desc;

typedef struct mi355_unet *mi355_unet_t;

typedef struct {
    int32_t patch[3];     /* (z,y,x), e.g. 128,128,128 */
    double step_size;     /* 0.5; a double, as nnU-Net forms patch * step from the Python float (4 bytes of padding before it) */
    int32_t use_gaussian; /* 1 */
    int32_t mirror_axes;  /* bit0 = z, bit1 = y, bit2 = x; 7 = 8-way TTA, 0 = no TTA */
    int32_t nonlin;       /* MI355_NONLIN_* applied to the logits of every forward */
    int32_t batch_tiles;  /* tiles per forward pass (0 = choose) */
} mi355_sw_opts;

const char *mi355_last_error(void);
int mi355_version(void);
/* number of visible gfx950 devices (0 if none / no HIP runtime device); other architectures are not counted */
int mi355_device_count(void);

int mi355_unet_create(const mi355_unet_desc *desc, mi355_unet_t *out);
int mi355_unet_destroy(mi355_unet_t net);
/* 2*MAC of every conv / transposed conv evaluated per forward of one [d,h,w] patch. */
int64_t mi355_unet_flops(mi355_unet_t net, int d, int h, int w);

/* x_dev: [n][in_channels][d][h][w] fp32 (NCDHW, as the reference module takes it).
 * logits_dev: [n][num_classes][d][h][w] fp32. */
int mi355_unet_forward(mi355_unet_t net, const float *x_dev, int n, int d, int h, int w,
                       float *logits_dev, void *stream);

/* Sliding-window prediction of one preprocessed volume.
 * vol_dev: [in_channels][Z][Y][X] fp32; probs_dev: [num_classes][Z][Y][X] fp32.
 * With n_nets > 1 the result is the arithmetic mean over the handles (folds), summed in
 * handle order (run_brats2021_inference_singlethread.py:128).
 * Asynchronous on `stream`: the work is enqueued, probs_dev is valid in stream order (a device fault surfaces at the
 * caller's next synchronisation, as with any HIP launch). */
int mi355_sw_predict(const mi355_unet_t *nets, int n_nets, const float *vol_dev, int Z, int Y, int X,
                     const mi355_sw_opts *opts, float *probs_dev, void *stream);
/* Host helper: the step table the predictor uses (nnU-Net v1 _compute_steps_for_sliding_window).
 * Writes at most max_steps entries, returns the count (or <0). */
int mi355_compute_steps(int patch, int image, double step_size, int32_t *steps, int max_steps);
/* Tile-sharded variant for multi-GPU: only tiles with (index % world) == rank are evaluated;
 * agg_dev [num_classes][Zp][Yp][Xp] receives the Gaussian-weighted partial sums (to be summed
 * across ranks in rank order), cnt_dev [Zp][Yp][Xp] the full normaliser. Zp.. = max(Z, patch). */
int mi355_sw_partial(mi355_unet_t net, const float *vol_dev, int Z, int Y, int X,
                     const mi355_sw_opts *opts, int rank, int world, float *agg_dev, float *cnt_dev,
                     void *stream);
int mi355_sw_finish(const float *agg_dev, const float *cnt_dev, int num_classes, int Z, int Y, int X,
                    const int32_t patch[3], float *probs_dev, void *stream);
/* The same with the reference's FOLD LIST (run_brats2021_inference_singlethread.py:161 folds=(0,1,2,3,4); :112-128 one
 * prediction per fold, np.mean over them): the work list is (fold, tile), item f * tiles + t, and item i belongs to rank
 * i % world.  agg_dev = sum over this rank's items of the Gaussian-weighted, mirror-averaged probabilities; the fold mean is
 * linear in the per-fold aggregates - mean_f(agg_f / cnt) = (sum_f agg_f) / cnt / n_folds - so ONE exchange of agg_dev per
 * ensemble member serves all folds (SURVEY.md 8e partitioning B: "(tile x mirror [x fold x model]) work list").
 * mi355_sw_finish_folds: probs = agg / cnt / n_folds on the rank-ordered sum of the partial aggregates (equals the per-fold
 * normalise-then-average of mi355_sw_predict up to fp32 rounding of the division order). */
int mi355_sw_partial_folds(const mi355_unet_t *nets, int n_nets, const float *vol_dev, int Z, int Y, int X,
                           const mi355_sw_opts *opts, int rank, int world, float *agg_dev, float *cnt_dev,
                           void *stream);
int mi355_sw_finish_folds(const float *agg_dev, const float *cnt_dev, int num_classes, int Z, int Y, int X,
                          const int32_t patch[3], int n_folds, float *probs_dev, void *stream);
/* Ensemble uncertainty.  run_brats2021_inference_singlethread.py:97-128 keeps the weighted mean of the samples (fold, covering tile,
 * mirror) of a voxel and nothing of their spread; these two keep the second moment beside it.  agg2_dev [num_classes][padded]
 * receives sum over this rank's items of gauss * (1 / n_mirrors) * sum_m p^2 - agg with p^2 in place of p, linear in the per-tile
 * terms, so it is summed over ranks exactly as agg is; agg_dev and cnt_dev are bit-identical to mi355_sw_partial_folds.
 * nonlin = identity has no probabilities: refused with MI355_ERR_INVALID. */
int mi355_sw_partial_folds_moments(const mi355_unet_t *nets, int n_nets, const float *vol_dev, int Z, int Y, int X,
                                   const mi355_sw_opts *opts, int rank, int world, float *agg_dev, float *agg2_dev,
                                   float *cnt_dev, void *stream);
/* mean_dev = agg / cnt / n_folds - bit-equal to mi355_sw_finish_folds - and m2_dev = agg2 / cnt / n_folds, both
 * [num_classes][Z][Y][X], cropped from the padded grid.  var = max(m2 - mean^2, 0) is derived by mi355_uncertainty_maps, after any
 * resampling of the two moments (an interpolation with non-negative weights keeps m2 >= mean^2 up to rounding). */
int mi355_sw_finish_moments(const float *agg_dev, const float *agg2_dev, const float *cnt_dev, int num_classes, int Z, int Y, int X,
                            const int32_t patch[3], int n_folds, float *mean_dev, float *m2_dev, void *stream);
/* Maps of one ensemble member (mean_b = m2_b = NULL) or of two with equal weight (mean = (a + b) / 2, m2 likewise: the moments over
 * the union of both members' samples); all inputs [C][Z][Y][X] fp32, C <= 8.  std = sqrt(max(m2 - mean^2, 0)); entropy in bits in
 * [0, 1] with 0 log 0 = 0: nonlin sigmoid - per channel -m log2 m - (1 - m) log2 (1 - m); nonlin softmax - per voxel
 * -sum_k m_k log2 m_k / log2 C, the same value in every channel.  std_dev / entropy_dev [C][Z][Y][X] (either may be NULL) receive the
 * per-channel maps; std_max_dev / entropy_max_dev [full] (either may be NULL) the maximum over channels, pasted at bbox_lo into a
 * zeroed volume as mi355_regions_to_labels pastes labels.  These replace, as a measurement, the literals of
 * feature_extraction/step5_quality.py:457-500 (calculate_measurement_confidence), which depend on nothing. */
int mi355_uncertainty_maps(const float *mean_a, const float *m2_a, const float *mean_b, const float *m2_b, int C, int Z, int Y, int X,
                           int nonlin, float *std_dev, float *entropy_dev, const int32_t bbox_lo[3], const int32_t full[3],
                           float *std_max_dev, float *entropy_max_dev, void *stream);
/* Per channel of mean_dev / var_dev / entropy_dev [C][n] (C <= 8) and n_thr <= 8 thresholds: counts_host [C][n_thr + 1] =
 * #{mean > t} per threshold (strict, as mi355_regions_to_labels), then |F| with F = {mean > 0.5}; sums_host [C][7] = the sums of
 * mean, var, entropy over all voxels, the same three over F, and max var.  fp64 sums in a fixed order (block partials, then an
 * ordered second stage; no atomics): bit-reproducible run to run.  Synchronises `stream`.  The numbers behind a volume interval and
 * a mean confidence where step5_quality.py:457-500 returns 'High' / 'Moderate'. */
int mi355_uncertainty_stats(const float *mean_dev, const float *var_dev, const float *entropy_dev, int C, int64_t n,
                            const float *thresholds_host, int n_thr, int64_t *counts_host, double *sums_host, void *stream);

/* seg = 0; for i in 0..C-1: seg[probs[i] > 0.5] = order[i]; pasted at bbox_lo into a zeroed
 * [full_z][full_y][full_x] uint8 volume.  order == NULL: seg = argmax over the C channels (first maximum wins), what
 * the same export does for trainers without regions (region_class_order=None). */
int mi355_regions_to_labels(const float *probs_dev, int C, int Z, int Y, int X, const int32_t *order,
                            const int32_t bbox_lo[3], const int32_t full[3], uint8_t *labels_dev,
                            void *stream);
/* out = uint8(round_half_even((a + b) / 2)) elementwise. */
int mi355_label_ensemble(const uint8_t *a_dev, const uint8_t *b_dev, uint8_t *out_dev, int64_t n,
                         void *stream);
/* probs_out = (a + b) / 2 (nnUNet_ensemble mode). */
int mi355_prob_mean(const float *a_dev, const float *b_dev, float *out_dev, int64_t n, void *stream);
/* Per channel: x[m] = (x[m]-mean(x[m]))/(std(x[m])+1e-8) ; x[~m] = 0  (m = mask != 0, ddof 0). */
int mi355_zscore_masked(float *vol_dev, const uint8_t *mask_dev, int C, int64_t voxels, void *stream);

/* ---- rows SURVEY.md 8f marks "next" (consumers of the label map / config 5's retrieval step) ---- */
/* out[i] = map[in[i]] (convert_labels_to_brats.py:34-55: nnU-Net {1,2,3} -> BraTS2025 {2,1,3} / BraTS2021 {2,1,4}). */
int mi355_label_remap(const uint8_t *in_dev, uint8_t *out_dev, int64_t n, const uint8_t *map256_host, void *stream);
/* counts_host[p*K+g] = #voxels with prediction p and ground truth g: everything evaluate_segmentation.py:12-49,
 * 129-195 derives (Dice, IoU, sensitivity, specificity per label and for WT/TC/ET) follows from these integers.
 * Bin K-1 is the "other" bin: it collects every label >= K-1, so pass K = (largest label of interest) + 2 and no
 * out-of-range label is ever counted as a real one; the K*K counts always sum to n.  2 <= K <= 8. */
int mi355_label_confusion(const uint8_t *pred_dev, const uint8_t *gt_dev, int64_t n, int K, uint64_t *counts_host,
                          void *stream);
/* scores = V @ q over L2-normalised rows, top-k by score (RAG_Assistant/rag_assistant.py:197-211).
 * vectors_dev [N][D] fp32, query_dev [D]; returns the number of results written (<= k) or < 0. */
int mi355_cosine_topk(const float *vectors_dev, const float *query_dev, int N, int D, int k, int32_t *idx_host,
                      float *scores_host, void *stream);

/* crop_to_nonzero of trainer.preprocess_patient (run_brats2021_inference_singlethread.py:89; nnU-Net v1
 * cropping.crop_to_nonzero): mask = OR_c(vol[c] != 0) with holes filled (scipy.ndimage.binary_fill_holes, 6-connectivity),
 * bbox_host = {z_lo, z_hi, y_lo, y_hi, x_lo, x_hi} (hi exclusive).  vol_dev [C][Z][Y][X] fp32, mask_dev [Z][Y][X] uint8.
 * Synchronous (returns the box). */
int mi355_crop_mask(const float *vol_dev, int C, int Z, int Y, int X, uint8_t *mask_dev, int32_t *bbox_host, void *stream);

/* Resampling between voxel grids (round 4): step 4 of trainer.preprocess_patient (run_brats2021_inference_singlethread.py:89 ->
 * nnU-Net v1 resample_patient: data order 3, mask order 1, a low-resolution axis separately with order 0) and the resampling inside
 * save_segmentation_nifti_from_softmax(..., order=1, force_separate_z=None, interpolation_order_z=0) (driver :131-138, :144-156).
 * One 1-D pass: in_dev viewed as [outer][n_in][inner] fp32 -> out_dev [outer][n_out][inner], sampled on the half-pixel-centred
 * grid x_in = (x_out + 0.5) * n_in / n_out - 0.5 with edge replication - what skimage.transform.resize(order, mode='edge',
 * anti_aliasing=False) / scipy.ndimage.zoom(order, mode='nearest', grid_mode=True) do along one axis.  order 0 (nearest), 1 (linear)
 * or 3 (cubic B-spline incl. its prefilter).  A tensor-product resize is one pass per axis, in any order.  Asynchronous on `stream`. */
int mi355_resize_axis(const float *in_dev, float *out_dev, int64_t outer, int n_in, int n_out, int64_t inner, int order,
                      void *stream);
/* x[g][0..n_per_group) clipped to [min, max] of ref[g][0..ref_per_group), g < groups (skimage's resize clips its output to the
 * range of its input image: per channel for a 3-D resize, per slice in nnU-Net's separate-z mode). */
int mi355_clip_to_range_of(float *x_dev, int64_t groups, int64_t n_per_group, const float *ref_dev, int64_t ref_per_group,
                           void *stream);
/* out[i] = x[i] >= thr (batchgenerators resize_segmentation: a label survives where its linearly resized indicator is >= 0.5;
 * here the inside-the-brain mask that use_mask_for_norm reads after resampling). */
int mi355_threshold_ge(const float *x_dev, float thr, uint8_t *out_dev, int64_t n, void *stream);
/* out[i] = mask[i] != 0 ? 1.0f : 0.0f (the indicator resize_segmentation resizes). */
int mi355_mask_to_float(const uint8_t *mask_dev, float *out_dev, int64_t n, void *stream);

/* Per-label voxel statistics of a label map [d0][d1][d2] (feature_extraction/utils.py:167-216: the integers behind
 * get_tumor_masks + calculate_volume + get_centroid + get_bounding_box).  stats_host[label * 10 + f], label < K <= 8:
 * f = 0 count, 1..3 sum of the coordinates along axis 0..2, 4..6 minimum, 7..9 maximum coordinate (-1 / 2^40 when the
 * label is absent; for label 0 only the count is filled).  Labels >= K are ignored.  Synchronous. */
int mi355_label_stats(const uint8_t *seg_dev, int d0, int d1, int d2, int K, int64_t *stats_host, void *stream);

/* Connected components of a binary volume [d0][d1][d2] (feature_extraction/step3_multiplicity.py:58-59 and :222-223:
 * scipy.ndimage.label(mask, generate_binary_structure(3, 3)); nnU-Net v1's post-processing labels with scipy's default structure).
 * Foreground = mask != 0.  connectivity 1 = 6 neighbours, 3 = 26 neighbours, anything else MI355_ERR_INVALID.  labels_dev [d0][d1][d2]
 * int32: 0 = background, components numbered 1..n in raster (C) order of their first voxel, which is scipy's numbering (the
 * reference's `id` fields and the tie order of its stable sort by volume, :112, :128, depend on it).  Union-find over voxel indices
 * in separate launches (csrc/components.hip); volumes of 2^31 voxels or more are refused.  Synchronous (returns n). */
int mi355_label_components(const uint8_t *mask_dev, int d0, int d1, int d2, int connectivity, int32_t *labels_dev,
                           int32_t *n_components_host, void *stream);
/* Per-component integers of a label map as mi355_label_components writes it (step3_multiplicity.py:63-121 and :227-242: what the
 * reference gets from `labeled_array == comp_id`, np.where and np.mean per component).  stats_host[(c - 1) * 14 + f] for component c:
 * f = 0 voxel count, 1..3 sum of the coordinates along axis 0..2, 4..6 minimum, 7..9 maximum coordinate, 10..13 number of its voxels
 * whose seg value is 1, 2, 3, 4 (seg_dev [d0][d1][d2] uint8, may be NULL: those four stay 0).  Exact and independent of arrival order.
 * n_components <= 65 536 (MI355_ERR_INVALID above, before anything is launched); labels beyond n_components are ignored.
 * Synchronous. */
int mi355_component_stats(const int32_t *labels_dev, const uint8_t *seg_dev, int d0, int d1, int d2, int n_components,
                          int64_t *stats_host, void *stream);
/* out[i] = keep[labels[i]] ? seg[i] : 0 for labels[i] in 1..n_components, out[i] = seg[i] elsewhere; keep_host has n_components + 1
 * entries, keep[0] is ignored (nnU-Net v1 remove_all_but_the_largest_connected_component: `image[(lmap == object_id) & mask] = 0`;
 * no counterpart in the reference tree).  out_dev may be seg_dev.  Asynchronous on `stream`. */
int mi355_component_filter(const int32_t *labels_dev, const uint8_t *seg_dev, int64_t n, const uint8_t *keep_host, int n_components,
                           uint8_t *out_dev, void *stream);
/* mi355_label_components with the neighbourhood named by its size: 6 (faces), 18 (faces and edges: scipy's
 * generate_binary_structure(3, 2), which step6_normal_structures.py:66-67 labels the CSF mask with) or 26 (corners too); anything
 * else MI355_ERR_INVALID.  Labels, numbering, limits and synchronisation as there. */
int mi355_label_components_nb(const uint8_t *mask_dev, int d0, int d1, int d2, int neighbours, int32_t *labels_dev,
                              int32_t *n_components_host, void *stream);

/* ---- binary morphology, distance transform and mask reductions (csrc/morphology.hip): the primitives under
 * feature_extraction/step4_morphology.py; step2_mass_effect.py:19,373 needs the first one too, step1_sequence_findings.py the
 * dilation, flag bits and moments, step5_quality.py (:408, :179-241, :283, :322-327) the erosion, flag bits, moments and centroid.  Volumes are [d0][d1][d2]
 * C-order with fewer than 2^31 voxels (MI355_ERR_INVALID otherwise), uint8 masks are foreground where nonzero, two calls give
 * bit-equal results, scratch is per stream lane. ---- */
/* scipy.ndimage.binary_erosion (dilate = 0) / binary_dilation (dilate != 0) with their defaults (step4_morphology.py:42, :149,
 * :227, :252, :254): the 6-neighbour cross, border_value = 0, `iterations` steps.  out_dev [d0][d1][d2] uint8 holds 0 / 1 and is
 * bit-equal to scipy's mask for every iterations >= 1.  Refused: iterations < 1 (scipy's "repeat until nothing changes"),
 * out_dev == mask_dev.  Asynchronous on `stream`. */
int mi355_binary_morphology(const uint8_t *mask_dev, int d0, int d1, int d2, int dilate, int iterations, uint8_t *out_dev,
                            void *stream);
/* Squared Euclidean distance, in voxel units, from every foreground voxel to the nearest background voxel of the volume; 0 on
 * the background (step4_morphology.py:160-161: scipy.ndimage.distance_transform_edt(mask) without `sampling`).  dist2_dev
 * [d0][d1][d2] int32 equals rint(distance_transform_edt(mask) ** 2) bit for bit: three separable integer passes, no rounding
 * anywhere.  Refused before any pass is launched: a volume without a background voxel (one counting launch and a 4-byte
 * read-back find that out, which makes the call synchronise once); (d0-1)^2 + (d1-1)^2 + (d2-1)^2 >= 2^31; d1 or d2 above
 * 1024 (a line of axis 1 or 2 must fit the 64 KiB LDS tile; axis 0 is scanned and has no such limit).  The passes themselves are
 * asynchronous on `stream`. */
int mi355_edt_squared(const uint8_t *mask_dev, int d0, int d1, int d2, int32_t *dist2_dev, void *stream);
/* |grad(sqrt(d2_in) - sqrt(d2_out))| at the voxels where surface_dev[i] & select is nonzero (select = 255: any nonzero
 * value), in fp64 with np.gradient's stencil - central difference / 2 inside, one-sided difference at the first and last index
 * of an axis (step4_morphology.py:163-181, which differentiates the whole volume and then indexes the surface).
 * stats_host[0..2] = number of surface voxels, mean, population standard deviation (all 0 when the surface is empty).  The
 * deviation comes from a second pass about the mean of the first; partial sums are combined in a fixed order.  Refused: an axis
 * shorter than 2, select outside 1..255.  Synchronous. */
int mi355_surface_gradient_stats(const int32_t *d2_in_dev, const int32_t *d2_out_dev, const uint8_t *surface_dev, int select,
                                 int d0, int d1, int d2, double *stats_host, void *stream);
/* moments_host[0..9] = n, sum c0, sum c1, sum c2, sum c0^2, sum c1^2, sum c2^2, sum c0 c1, sum c0 c2, sum c1 c2 over the
 * foreground voxels (c_k = index along axis k): what calculate_elongation (step4_morphology.py:78-115) reduces np.where(mask)
 * to.  Exact int64, independent of arrival order.  Synchronous. */
int mi355_mask_second_moments(const uint8_t *mask_dev, int d0, int d1, int d2, int64_t *moments_host, void *stream);
/* vols_dev [C][n] fp32, flags_dev [n] uint8 whose 8 bits mark 8 regions that may overlap.  out_host[(b * C + c) * 3 + 0..2] =
 * number of voxels with bit b, sum and sum of squares over them of channel c, accumulated in fp64 in a fixed order (the
 * boolean-mask indexing, .mean() and .std() of step4_morphology.py:231-262 and :324-338).  Sums of integer-valued volumes are
 * exact while they stay below 2^53.  Refused: C outside 1..8, n outside 1..2^31-1.  Synchronous. */
int mi355_masked_moments(const float *vols_dev, int C, const uint8_t *flags_dev, int64_t n, double *out_host, void *stream);
/* Bit `bit` (0..7) of flags_dev[i] = set256_host[labels_dev[i]] != 0; the other bits stay (utils.py:167-178 get_tumor_masks;
 * with a 0 / 1 mask as the label map and the set {1}: a mask becomes a bit).  Asynchronous on `stream`. */
int mi355_flag_from_labels(const uint8_t *labels_dev, const uint8_t *set256_host, int bit, uint8_t *flags_dev, int64_t n,
                           void *stream);
/* Bit `bit` of flags_dev[i] = every bit of `require` is set, no bit of `forbid` is, and - when x_dev is not NULL -
 * lo < (double)x_dev[i] < hi; computed from the byte as it was, so `bit` may be among require / forbid.  lo, hi are fp64, +-inf
 * allowed, NaN refused (the `dilated & ~mask` bands of step4_morphology.py:228, :253-254 and the CSF-like predicate of
 * :329-333, chained over T1, T2 and FLAIR).  Asynchronous on `stream`. */
int mi355_flag_from_flags(uint8_t *flags_dev, int bit, int require, int forbid, const float *x_dev, double lo, double hi, int64_t n,
                          void *stream);

/* ---- exact masked order statistics (csrc/percentile.hip): what the reference sorts for np.percentile (utils.py:48-49, :57, :67;
 * step2_mass_effect.py:179; step4_morphology.py:317-320; step5_quality.py:194-212; step6_normal_structures.py:48-50, :129, :313).  On the device: steps 1, 2, 4, 5
 * and 6 (brats_amd.sequence_findings, .mass_effect, .morphology, .quality, .normal_structures) ---- */
/* Voxel i of x_dev [n] fp32 takes part when (flags_dev is NULL, or every bit of `require` is set in flags_dev[i] and no bit of
 * `forbid` is) and lo < (double)x_dev[i] < hi - the selection of mi355_flag_from_flags; lo, hi fp64, +-inf allowed, so
 * `data[data > 0]` is lo = 0, hi = +inf.  A NaN never passes the comparison.  count_host[0] = m, the number of voxels that take
 * part; count_host[1] = the number of NaN among the voxels the flag test alone selects (numpy would have returned NaN: the
 * caller decides).  For each percentile q_host[j] in [0, 100], with v = (m - 1) * (q / 100) in IEEE double as numpy forms it:
 * below_host[j] = the ascending order statistic of rank floor(v), above_host[j] = the one of rank min(floor(v) + 1, m - 1); both
 * are fp32 values of the volume, exact (-0.0 counts as and is returned as +0.0).  np.percentile's linear interpolation is host
 * arithmetic on the two.  m = 0 leaves below_host / above_host untouched and succeeds.  Radix select on the order-preserving
 * key of the float, four histogram passes over x_dev and flags_dev (5 bytes per voxel each), no sort, no copy of the selected
 * values; up to 8 percentiles share every pass.  Counters meet in integer atomics: two calls are bit-equal.  Scratch is per
 * stream lane.  Refused: nq outside 1..8, a q outside [0, 100] or NaN, n outside 1..2^31-1, a NaN bound, require or forbid
 * outside 0..255 or sharing a bit.  Synchronous. */
int mi355_masked_percentiles(const float *x_dev, int64_t n, const uint8_t *flags_dev, int require, int forbid, double lo, double hi,
                             const double *q_host, int nq, int64_t *count_host, float *below_host, float *above_host, void *stream);
/* mi355_masked_percentiles for nvol = 1..4 volumes x_dev[v] [n] fp32 that share flags_dev: the reference's six steps take the same
 * percentiles again and again (the positive voxels of each modality: utils.py:57, :67, step4_morphology.py:317-320,
 * step5_quality.py:194; the brain's: step2_mass_effect.py:179, step5_quality.py:210-212, step6_normal_structures.py:48-50), and
 * feature_extraction/run_all.py:411-446 runs all six on one case.  Volume v has its own require[v], forbid[v], lo[v], hi[v] and
 * its own nq[v] = 1..8 percentiles q_host[v][0..nq[v]).  count_host[2 v], count_host[2 v + 1], below_host[8 v + j] and
 * above_host[8 v + j] are what mi355_masked_percentiles returns for that volume alone, bit for bit; a volume that selects nothing
 * leaves its below / above untouched and does not keep the others from being selected.  Each of the four passes is one launch
 * over the voxels and one read-back for all volumes: a thread loads the flag byte once and the word of a volume only when the byte
 * passes that volume's flag test.  LDS is sized by the prefixes that are live in the pass; where they exceed what the device
 * allows a workgroup, the pass is split by volume into several launches ahead of the one read-back.  launches_host (NULL allowed)
 * receives the number of launches: 4 when no pass was split and every volume selects something.  Refused: nvol outside 1..4, an
 * nq[v] outside 1..8, a q outside [0, 100] or NaN, n outside 1..2^31-1, a NaN bound, require[v] or forbid[v] outside 0..255 or
 * sharing a bit - all before anything is launched.  Synchronous. */
int mi355_masked_percentiles_multi(const float *const *x_dev, int nvol, int64_t n, const uint8_t *flags_dev, const int *require, const int *forbid,
                                   const double *lo, const double *hi, const double *const *q_host, const int *nq, int64_t *count_host,
                                   float *below_host, float *above_host, int *launches_host, void *stream);

/* ---- hole filling, Sobel gradient statistics, radial shells and face slabs (csrc/quality.hip): the primitives under
 * feature_extraction/step5_quality.py that the entries above do not cover.  Conventions as for csrc/morphology.hip: volumes are
 * [d0][d1][d2] C-order with fewer than 2^31 voxels (MI355_ERR_INVALID otherwise), uint8 masks are foreground where nonzero, two
 * calls give bit-equal results (fp64 sums are combined in a fixed order, integers meet in integer atomics), scratch is per
 * stream lane. ---- */
/* scipy.ndimage.binary_fill_holes(mask) with its default structure (step5_quality.py:103): a background voxel stays background
 * exactly when a path of 6-neighbour steps through background voxels joins it to a voxel on one of the six faces of the volume.
 * out_dev [d0][d1][d2] uint8 holds 0 / 1 and is bit-equal to scipy's result; *filled_host = the number of voxels added.  The
 * complement is labelled by mi355_label_components at connectivity 1 (one union-find labelling, no sweep that repeats until
 * nothing changes), the components that own a face voxel are marked, and the others are filled.  Refused: out_dev == mask_dev.
 * Synchronous. */
int mi355_binary_fill_holes(const uint8_t *mask_dev, int d0, int d1, int d2, uint8_t *out_dev, int64_t *filled_host, void *stream);
/* sqrt(gx^2 + gy^2 + gz^2) in fp64 at the voxels where flags_dev[i] & select is nonzero, g_axis being
 * scipy.ndimage.sobel(x.astype(float), axis) with scipy's defaults (step5_quality.py:413-416, which differentiates the whole
 * volume and then indexes the tumour edge): [-1, 0, 1] along the axis, [1, 2, 1] along each of the other two, boundary mode
 * `reflect` (index -1 reads index 0, index n reads index n - 1; an axis of length 1 reads itself).  A 27-point gather at the
 * selected voxels only.  stats_host[0..2] = number of selected voxels, mean, population standard deviation (all 0 when nothing
 * is selected); the deviation comes from a second pass about the mean of the first.  For integer-valued x below 2^15 every
 * magnitude is the correctly rounded root of an exact integer, bit-equal to scipy's.  Refused: select outside 1..255.
 * Synchronous. */
int mi355_sobel_magnitude_stats(const float *x_dev, const uint8_t *flags_dev, int select, int d0, int d1, int d2, double *stats_host,
                                void *stream);
/* Over the voxels whose flag byte has every bit of `require` (step5_quality.py:280-300): out_host[0] = max_dist, the maximum of
 * sqrt((c0 - centre[0])**2 + (c1 - centre[1])**2 + (c2 - centre[2])**2) evaluated in fp64 in that order, every square rounded
 * before the additions (no fused multiply-add); out_host[1], [2] = the number and the fp64 sum of x over the voxels with
 * dist < max_dist * inner_frac; out_host[3], [4] = the same over the voxels with dist > max_dist * outer_frac.  An empty
 * selection gives all zeros and succeeds.  Refused: require outside 0..255, a NaN centre or fraction.  Synchronous. */
int mi355_radial_shell_moments(const float *x_dev, const uint8_t *flags_dev, int require, int d0, int d1, int d2, const double centre[3],
                               double inner_frac, double outer_frac, double *out_host, void *stream);
/* counts_host[2 a], counts_host[2 a + 1] = the number of voxels with x > 0 among the first `margin` and among the last `margin`
 * indices of axis a (step5_quality.py:385-390: `t1_data[:5].max() > 0` is counts_host[0] > 0); a margin at or above the axis
 * length means the whole axis.  A NaN is not counted.  Refused: margin < 1.  Synchronous. */
int mi355_face_slab_counts(const float *x_dev, int d0, int d1, int d2, int margin, int64_t *counts_host, void *stream);

/* ---- axis profiles, box counts, ranked picks, point-set distance and a masked minimum (csrc/mass_effect.hip): the primitives under
 * feature_extraction/step2_mass_effect.py that the entries above do not cover.  Conventions as for csrc/morphology.hip and
 * csrc/quality.hip: volumes are [d0][d1][d2] C-order with fewer than 2^31 voxels (MI355_ERR_INVALID otherwise); a voxel is
 * SELECTED when every bit of `require` is set in flags_dev[i] and no bit of `forbid` is (both in 0..255, sharing no bit - the
 * selection of mi355_flag_from_flags); two calls give bit-equal results (integers meet in integer atomics, there is no float
 * anywhere); scratch is per stream lane; null pointers and sizes out of range are refused before anything is launched. ---- */
#define MI355_AXIS_COUNTS_MAX 4096  /* longest axis of mi355_axis_counts: its d0 + d1 + d2 32-bit counters must fit 48 KiB of LDS */
#define MI355_MAX_BOXES 16
#define MI355_MAX_POINTS 65536
/* counts_host[0 .. d0), [d0 .. d0 + d1), [d0 + d1 .. d0 + d1 + d2) = the number of selected voxels at each index of axis 0, 1, 2.
 * Host arithmetic gets from them what step2_mass_effect.py takes from np.where(mask): `brain_coords[0].min() / .max()` (:66-67),
 * `tumor_coords[0].mean()` (:73; an exact integer sum divided once), `left_half.sum()`, `right_half.sum()` and
 * `ndimage.center_of_mass(half)[0]` (:84-93), the CSF halves (:186-193), `tumor_mask[:k].sum()` (:447-448), utils.get_centroid and
 * utils.get_bounding_box (:441-442).  Refused: an axis longer than MI355_AXIS_COUNTS_MAX.  Synchronous. */
int mi355_axis_counts(const uint8_t *flags_dev, int require, int forbid, int d0, int d1, int d2, int64_t *counts_host, void *stream);
/* counts_host[b] = the number of selected voxels with lo_k <= c_k < hi_k on every axis k, for the nb (1..MI355_MAX_BOXES) boxes
 * boxes_host[b * 6 + 0..5] = lo0, hi0, lo1, hi1, lo2, hi2: `(tumor_mask & lobe_mask).sum()` of step2_mass_effect.py:472-518, whose
 * lobe masks are slices (the temporal lobe is two boxes).  Boxes may overlap; a box with lo >= hi on an axis counts 0.  Refused:
 * lo < 0 or hi > the axis length.  Synchronous. */
int mi355_box_counts(const uint8_t *flags_dev, int require, int forbid, int d0, int d1, int d2, const int32_t *boxes_host, int nb,
                     int64_t *counts_host, void *stream);
/* count_host[0] = m, the number of selected voxels among flags_dev[0 .. n); index_dev[j] = the linear index of the selected voxel
 * whose 0-based rank among the selected voxels in C order is ranks_host[j], i.e. np.flatnonzero(selected)[ranks] - what
 * `tumor_coords[k][sample_idx]` and `csf_points[csf_sample_idx]` of step2_mass_effect.py:215-225 index, without np.where.  Ranks
 * come in any order and may repeat; 1 <= k <= MI355_MAX_POINTS; n in 1..2^31-1.  One count per 4096-voxel block, a two-level
 * scan of the counts, then one wave per rank finds the owning block by bisection and the voxel by popcounts and a wave scan.
 * A rank outside [0, m) fails the call with nothing written to index_dev; count_host is filled all the same.  Synchronous. */
int mi355_select_ranked(const uint8_t *flags_dev, int require, int forbid, int64_t n, const int64_t *ranks_host, int k,
                        int64_t *index_dev, int64_t *count_host, void *stream);
/* min_host[0] = the smallest squared Euclidean distance, in voxel units, between a voxel of a_index_dev [ka] and one of
 * b_index_dev [kb] (linear C-order indices into [d0][d1][d2], as mi355_select_ranked writes them; ka, kb in
 * 1..MI355_MAX_POINTS): the double loop of step2_mass_effect.py:227-232.  An exact integer; sqrt is monotone and correctly
 * rounded, so sqrt(min d^2) is the reference's min(sqrt(d^2)) bit for bit.  Refused after the launch, with min_host untouched: an
 * index outside the volume (the kernel reads the two lists and nothing else).  Synchronous. */
int mi355_min_pair_dist2(const int64_t *a_index_dev, int ka, const int64_t *b_index_dev, int kb, int d0, int d1, int d2,
                         int64_t *min_host, void *stream);
/* min_host[0] = the minimum of values_dev [n] int32 over the selected voxels, count_host[0] = their number; an empty selection
 * leaves min_host untouched and succeeds with count 0.  With mi355_edt_squared of the complement of a mask as the values this is
 * the exact squared distance from the selection to that mask: the minimum over ALL pairs of what step2_mass_effect.py:214-232
 * samples.  n in 1..2^31-1.  Synchronous. */
int mi355_masked_min_i32(const int32_t *values_dev, const uint8_t *flags_dev, int require, int forbid, int64_t n, int32_t *min_host,
                         int64_t *count_host, void *stream);

/* ---- city-block distance, integer flag predicates, int32 order statistics and a column-count maximum
 * (csrc/normal_structures.hip): the primitives under feature_extraction/step6_normal_structures.py that the entries above do not
 * cover.  Conventions as for csrc/morphology.hip and csrc/mass_effect.hip: volumes are [d0][d1][d2] C-order with fewer than 2^31
 * voxels (MI355_ERR_INVALID otherwise), uint8 masks are foreground where nonzero, two calls give bit-equal results (there is no
 * float anywhere: a voxel has one writer, reductions meet in integer atomics), scratch is per stream lane. ---- */
#define MI355_CITYBLOCK_FAR 1073741824u  /* 2^30: the distance mi355_cityblock_distance writes where there is nothing to measure to */
/* The exact city-block (L1, taxicab) distance transform: what scipy.ndimage.binary_dilation / binary_erosion with their default
 * cross reach in `iterations` steps, for every number of steps at once (step6_normal_structures.py:152 dilates the tumour 5 steps,
 * :345 the same mask 10 steps, :215 the ventricles 10 steps; :62-63 and :272 erode).  dist_dev [d0][d1][d2] int32:
 *   to_foreground != 0: the distance to the nearest nonzero voxel of the mask, 0 on it, MI355_CITYBLOCK_FAR everywhere when the
 *     mask is empty; `dist <= n` is bit-equal to binary_dilation(mask, iterations=n) for every n >= 1;
 *   to_foreground == 0: the distance to the nearest zero voxel, every position outside the volume counting as zero (scipy's
 *     border_value = 0), so a volume without a zero voxel holds its distances to the faces; `dist > n` is bit-equal to
 *     binary_erosion(mask, iterations=n).
 * Three separable passes in place, each a forward and a backward running minimum along its axis.  Refused: d0 + d1 + d2 above
 * 2^30, d2 above 16383 (a line of axis 2 must fit the 64 KiB LDS tile).  Asynchronous on `stream`. */
int mi355_cityblock_distance(const uint8_t *mask_dev, int d0, int d1, int d2, int to_foreground, int32_t *dist_dev, void *stream);
/* Bit `bit` (0..7) of flags_dev[i] = every bit of `require` is set, no bit of `forbid` is, and lo <= values_dev[i] <= hi (both
 * ends included); computed from the byte as it was.  The integer twin of mi355_flag_from_flags: `dist <= 5` on a city-block map
 * (step6_normal_structures.py:152-153, :215-216, :345-346) and `brain_dist > threshold` / `< threshold` on the squared distance
 * map of mi355_edt_squared, the float threshold turned into an integer bound on d^2 by the caller (:210, :224).  Asynchronous on
 * `stream`. */
int mi355_flag_from_i32(uint8_t *flags_dev, int bit, int require, int forbid, const int32_t *values_dev, int32_t lo, int32_t hi, int64_t n,
                        void *stream);
/* Bit `bit` of flags_dev[i] = every bit of `require` is set, no bit of `forbid` is, and the voxel lies inside the half-open index
 * box box_host[0..5] = lo0, hi0, lo1, hi1, lo2, hi2, which is clipped to the volume (lo >= hi on an axis: nowhere):
 * `inferior_brain[:, :, inferior_third:] = False` of step6_normal_structures.py:306-308 is the box [0, d0) x [0, d1) x [0, d2 / 3).
 * Asynchronous on `stream`. */
int mi355_flag_from_box(uint8_t *flags_dev, int bit, int require, int forbid, int d0, int d1, int d2, const int32_t *box_host, void *stream);
/* mi355_masked_percentiles for an int32 map with values in [0, 2^31): count_host[0] = m, the number of voxels whose flag byte has
 * every bit of `require` and no bit of `forbid` (flags_dev NULL: all n), and per percentile q_host[j] the two exact order
 * statistics of rank floor(v) and min(floor(v) + 1, m - 1), v = (m - 1) * (q / 100), in below_host[j] / above_host[j] (untouched
 * when m = 0).  step6_normal_structures.py:207 and :224 take np.percentile(brain_dist[brain_mask], 60) and the 40th of
 * distance_transform_edt, the root of exact integers: the root is monotone, so the host takes np.sqrt of the two order statistics
 * of mi355_edt_squared's map and interpolates as numpy does.  The radix select of csrc/percentile.hip on the value as its own key.
 * Refused: a negative selected value, nq outside 1..8, a q outside [0, 100] or NaN, n outside 1..2^31-1, require or forbid
 * outside 0..255 or sharing a bit.  Synchronous. */
int mi355_masked_order_stats_i32(const int32_t *values_dev, int64_t n, const uint8_t *flags_dev, int require, int forbid, const double *q_host,
                                 int nq, int64_t *count_host, int32_t *below_host, int32_t *above_host, void *stream);
/* out_host[0] = np.max(np.sum(selected[:, i1_from:, :], axis=0)) (step6_normal_structures.py:130-131: the widest run of ventricle
 * voxels along axis 0 in front of `frontal_y`), selected as for mi355_axis_counts; 0 when i1_from >= d1 or nothing is selected
 * there.  Refused: i1_from < 0.  Synchronous. */
int mi355_column_count_max(const uint8_t *flags_dev, int require, int forbid, int d0, int d1, int d2, int i1_from, int64_t *out_host, void *stream);

/* ---- surface distances between two label maps (csrc/surface_distance.hip): what brats_amd.evaluate derives the 95 % Hausdorff
 * distance, the average symmetric surface distance and the surface Dice from (MedPy's definitions, which nnU-Net v1's evaluator
 * reports beside Dice).  Volumes are [d0][d1][d2] C-order with fewer than 2^31 voxels; a box is lo_host[3] <= index < hi_host[3]
 * inside the volume, and a box-shaped map is dense over it, [hi0 - lo0][hi1 - lo1][hi2 - lo2].  None of the three takes device
 * scratch: all working memory is the caller's, passed with its size, and no result depends on what it held before the call. ---- */
#define MI355_SURFACE_EDT_MAX_LINE 512 /* longest axis 1 / axis 2 of a box of mi355_edt_to_flagged_f64: a [512][8] fp64 tile is its 32 KiB of LDS */
#define MI355_GATHER_CHUNK 2048        /* box voxels per block count of mi355_gather_flagged_f64 */
/* One pass over both label maps.  pred_table256_host / gt_table256_host [256]: label value -> mask of the regions (bits 0..3) the
 * label belongs to in that map; an entry above 15 is refused.  flags_dev [d0][d1][d2] uint8 (flags_bytes >= the voxel count, must
 * not alias a label map): bit r = the voxel is on the surface of region r of the prediction, bit 4 + r the same for the ground
 * truth, where surface = mask & ~binary_erosion(mask) with scipy's defaults (6-neighbour cross, one iteration, border_value = 0:
 * a position outside the volume counts as background).  Every byte is written.  Asynchronous on `stream`. */
int mi355_region_surfaces(const uint8_t *pred_dev, const uint8_t *gt_dev, int d0, int d1, int d2, const uint8_t *pred_table256_host,
                          const uint8_t *gt_table256_host, uint8_t *flags_dev, int64_t flags_bytes, void *stream);
/* dist2_dev (box-shaped fp64, dist2_capacity >= the box's voxel count) = for every voxel x of the box the minimum over the sites y
 * - the voxels of the box with flags_dev[y] & select != 0 - of ((x0-y0) s0)^2 + ((x1-y1) s1)^2 + ((x2-y2) s2)^2, s = spacing_host[3],
 * each product, square and sum rounded once in fp64 and the terms added in this order: the square of
 * scipy.ndimage.distance_transform_edt(~sites, sampling=spacing) on the box.  Sites outside the box are ignored.  count_dev: one
 * 32-bit device word of working memory.  Refused before any pass is launched: a box without a site (one counting launch and a 4-byte
 * read-back find that out, which makes the call synchronise once), axis 1 or 2 of the box longer than MI355_SURFACE_EDT_MAX_LINE
 * (axis 0 is scanned and has no such limit), select outside 1..255, a spacing that is not finite and positive, a map that is too
 * small.  The passes themselves are asynchronous on `stream`. */
int mi355_edt_to_flagged_f64(const uint8_t *flags_dev, int d0, int d1, int d2, const int32_t *lo_host, const int32_t *hi_host, int select,
                             const double *spacing_host, double *dist2_dev, int64_t dist2_capacity, uint32_t *count_dev, void *stream);
/* out_dev[0 .. count) = values_dev (box-shaped fp64) at the voxels of the box with flags_dev & select != 0, in raster order of the
 * box; *count_host = their number.  Order and count follow from the inputs alone: a count per MI355_GATHER_CHUNK voxels, an exclusive
 * scan, a scatter to computed positions.  block_counts_dev: block_words >= ceil(box voxels / MI355_GATHER_CHUNK) + 1 32-bit device
 * words of working memory.  count > capacity is an error, not a truncation: *count_host is set and nothing is written to out_dev.
 * out_dev NULL (with capacity 0; values_dev may be NULL too): a count-only call.  Synchronises once, for the count; the scatter is asynchronous on `stream`. */
int mi355_gather_flagged_f64(const double *values_dev, const uint8_t *flags_dev, int d0, int d1, int d2, const int32_t *lo_host,
                             const int32_t *hi_host, int select, double *out_dev, int64_t capacity, uint32_t *block_counts_dev,
                             int64_t block_words, int64_t *count_host, void *stream);

/* ---- lesion-wise scoring (csrc/lesionwise.hip): the three pieces brats_amd.evaluate.lesionwise_metrics needs beside the labelling
 * above and the surface-distance entry points - the BraTS 2023+ ranking scores a prediction per lesion (the ground truth dilated,
 * its components grouped into lesions, predicted components matched to them).  Volumes are [d0][d1][d2] C-order with fewer than 2^31
 * voxels.  None of the four takes device scratch: all working memory is the caller's, passed with its size, and no result depends
 * on what it held before the call.  Integers only: two calls give bit-equal results.  A refused call writes to no output. ---- */
#define MI355_MORPH_NB_BRICK0 8        /* output voxels of one workgroup of mi355_binary_morphology_nb along axis 0, 1, 2 */
#define MI355_MORPH_NB_BRICK1 16
#define MI355_MORPH_NB_BRICK2 64
#define MI355_MORPH_NB_LDS_STEPS 4     /* steps one launch runs on bit-planes in LDS (= the halo it stages); more iterations are several launches */
#define MI355_PAIR_TABLE_MAX 1048576   /* most entries (n_a + 1) * (n_b + 1) of mi355_label_pair_counts */
#define MI355_PAIR_LDS_BINS 8192       /* the first so many entries of a table are counted in LDS per workgroup, the rest in global memory */
#define MI355_LOOKUP_MAX_LABEL 65536   /* largest n of mi355_label_lookup / _i32 */
/* scipy.ndimage.binary_erosion (dilate = 0) / binary_dilation (dilate != 0)(mask, generate_binary_structure(3, c), iterations,
 * border_value = 0) with c = 1, 2, 3 named by `neighbours` = 6, 18, 26: out_dev [d0][d1][d2] uint8 holds 0 / 1 and is bit-equal to
 * scipy's mask for every iterations >= 1 (a position outside the volume counts as 0 in every step).  Up to MI355_MORPH_NB_LDS_STEPS
 * iterations are one launch and tmp_dev may be NULL; more are ceil(iterations / MI355_MORPH_NB_LDS_STEPS) launches that alternate
 * between out_dev and tmp_dev (tmp_bytes >= the voxel count; neither may alias the other or the input).  Refused: iterations < 1,
 * another neighbourhood, aliased buffers, a missing or short tmp_dev when it is needed.  Asynchronous on `stream`. */
int mi355_binary_morphology_nb(const uint8_t *mask_dev, int d0, int d1, int d2, int dilate, int neighbours, int iterations, uint8_t *out_dev,
                               uint8_t *tmp_dev, int64_t tmp_bytes, void *stream);
/* counts_host[a * (n_b + 1) + b] = the voxels i < V with labels_a[i] == a and labels_b[i] == b, a = 0..n_a, b = 0..n_b: numpy's
 * np.add.at(table, (labels_a, labels_b), 1), which replaces one `np.isin` / `labelled == id` pass per component.  The table sums to
 * V.  table_dev: table_words >= (n_a + 1) * (n_b + 1) + 1 64-bit device words of working memory (cleared by the call).  Refused by
 * return code, with counts_host untouched: a table of more than MI355_PAIR_TABLE_MAX entries (the message names n_a and n_b), too
 * few table_words, a voxel whose label lies outside 0..n_a / 0..n_b (such a label is counted, never used as an index).  Synchronous. */
int mi355_label_pair_counts(const int32_t *labels_a_dev, int n_a, const int32_t *labels_b_dev, int n_b, int64_t V, int64_t *table_dev,
                            int64_t table_words, int64_t *counts_host, void *stream);
/* out_dev[i] = table_host[labels_dev[i]] for i < V, table_host[0] included: numpy's table[labels], n + 1 entries of uint8 (_i32: of
 * int32), n <= MI355_LOOKUP_MAX_LABEL.  work_dev: work_bytes >= 16 + (n + 1) * the entry size bytes of device working memory (a count
 * word and the table's copy; the entry points have no other way to a device table without library-owned memory).  One launch looks
 * for labels outside 0..n first (a 4-byte read-back: the call synchronises once); if there is one the call is refused and out_dev is
 * untouched.  out_dev must not be labels_dev.  The lookup itself is asynchronous on `stream`. */
int mi355_label_lookup(const int32_t *labels_dev, int64_t V, int n, const uint8_t *table_host, void *work_dev, int64_t work_bytes, uint8_t *out_dev,
                       void *stream);
int mi355_label_lookup_i32(const int32_t *labels_dev, int64_t V, int n, const int32_t *table_host, void *work_dev, int64_t work_bytes,
                           int32_t *out_dev, void *stream);

/* ---- the resident case (csrc/resident_case.hip): what brats_amd.pipeline needs to hand the case the inference driver holds - file
 * order, [C][Z][Y][X] - to the evaluator and the feature steps, which take [x][y][z] volumes, without a trip through the host. ---- */
#define MI355_REVERSE_AXES_MAX_ELEMENTS 2147483648ll   /* channels * d0 * d1 * d2 stays below this */
/* dst[c][k][j][i] = src[c][i][j][k]: src_dev [channels][d0][d1][d2] -> dst_dev [channels][d2][d1][d0], both contiguous, elements of
 * elem_bytes = 1 (label maps) or 4 (float32 volumes) bytes, moved bit for bit (NaN payloads included).  Any d0, d1, d2 >= 1; a
 * pointer need only be aligned to its element (a slice of a larger tensor).  Takes no device scratch and is asynchronous on
 * `stream`.  Refused (MI355_ERR_INVALID, nothing is launched, dst_dev is not written): a null pointer, a dimension below 1,
 * another elem_bytes, MI355_REVERSE_AXES_MAX_ELEMENTS elements or more, source and destination that overlap, a pointer to 4-byte
 * elements that is not aligned to 4 bytes. */
int mi355_reverse_axes(const void *src_dev, void *dst_dev, int channels, int d0, int d1, int d2, int elem_bytes, void *stream);

/* Device scratch, for tests (DESIGN.md "Scratch holds no state").  Working memory lives in slots (csrc/common.h, enum ScratchSlot;
 * ops.SCRATCH_SLOTS names them in that order), one set per stream lane; the first MI355_SCRATCH_LANES distinct streams get a lane
 * each, a further stream takes over the least recently used one.  The two zero pages (slots 4 and 5) are shared by all lanes.
 * A result never depends on what a slot held on entry: these four let a test put something there.  Host code, no kernels. */
#define MI355_SCRATCH_LANES 4
/* bytes[i] = bytes now allocated for slot i, i < min(n, slot count), for the lane of `stream` (zero pages: the shared ones).
 * Allocates nothing and claims no lane: a stream without a lane reports 0 for the lane-owned slots.  Returns the slot count. */
int mi355_scratch_sizes(void *stream, int64_t *bytes, int n);
/* hipMemsetD32Async(word) on `stream` over the whole buffer of `slot` of the stream's lane; slot = -1: every lane-owned slot of
 * the lane.  Returns the bytes filled (0: no lane, or nothing allocated).  Refused: a zero page, a slot out of range. */
int64_t mi355_scratch_fill(void *stream, int slot, uint32_t word);
/* Synchronises the device, frees the lane-owned buffers of the stream's lane and forgets the lane: the next request on that
 * stream claims a lane and allocates afresh.  A stream without a lane: nothing happens. */
int mi355_scratch_release(void *stream);
/* nonzero_bytes[0], [1] = the number of non-zero bytes in the two shared zero pages (0 for a page that does not exist yet),
 * after a device synchronise. */
int mi355_scratch_zero_pages(int64_t *nonzero_bytes);
/* Device memory that is not scratch - the weights of every live handle, their Gaussian maps, and for the length of a call the
 * buffers and weights of a single-op entry point - has one owner per handle or call; *count / *bytes = the allocations and bytes
 * all owners of this process hold now.  A handle that was destroyed, a create that was refused and a call that has returned hold
 * none.  Host code, needs no device. */
int mi355_live_allocations(int64_t *count, int64_t *bytes);

/* Per-kernel timing with HIP events on the stream the kernels are launched on (bench.py's
 * roofline). flops / bytes are the ALGORITHMIC work of the recorded launches. */
typedef struct {
    char name[64];
    int64_t launches;
    double ms, flops, bytes;
} mi355_prof_entry;
int mi355_profile_enable(mi355_unet_t net, int on);
int mi355_profile_read(mi355_unet_t net, mi355_prof_entry *out, int max_entries);

/* Single-op entry points (used by the parity tests; same kernels the network runs).
 * NDHWC fp32 device tensors. act: 0 none, 1 LeakyReLU(slope). */
int mi355_conv3d_ndhwc(const float *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                       const float *bias_host, int cout, int stride, int act, float slope, int impl,
                       float *y_dev, void *stream);
int mi355_tconv3d_ndhwc(const float *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                        int cout, float *y_dev, void *stream);
/* fp16-storage variants: x_dev / y_dev hold IEEE half plain NDHWC tensors (cin % 16 == 0, cout % 32 == 0); inside the library
 * fp16 activations are channel-blocked ([N][C/8][D][H][W][8]) and these entry points convert on the way in and out.  They
 * (these two, mi355_conv3d_sums_ndhwc and mi355_conv3d_fused_ndhwc with fp16) keep the kernel's channel-blocked output
 * between two guard bands and return MI355_ERR_HIP, with the byte counts in mi355_last_error, if the launch changed either. */
int mi355_conv3d_ndhwc_f16(const void *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                           const float *bias_host, int cout, int stride, int act, float slope, void *y_dev,
                           void *stream);
int mi355_tconv3d_ndhwc_f16(const void *x_dev, int n, int d, int h, int w, int cin, const float *weight_host,
                            int cout, void *y_dev, void *stream);
/* One convolution WITH the run-time-norm statistics epilogue: y = act(conv(x) + b) as mi355_conv3d_ndhwc[_f16] (dtype =
 * MI355_F32 / MI355_F16; plain NDHWC operands of that dtype; the kernel the network would dispatch for this shape), and
 * sums_dev[n][cout][2] = (sum over voxels of y, sum of y^2) in fp64 - the two numbers nn.InstanceNorm3d / nn.GroupNorm in
 * ConvDropoutNormNonlin (generic_UNet.py:62-72) reduce their input to, accumulated by the conv kernel's epilogue from the
 * fp32 values BEFORE any rounding to fp16.  Test aid for the statistics instantiations of every conv kernel. */
int mi355_conv3d_sums_ndhwc(const void *x_dev, int dtype, int n, int d, int h, int w, int cin, const float *weight_host,
                            const float *bias_host, int cout, int stride, int act, float slope, void *y_dev,
                            double *sums_dev, void *stream);
/* One convolution with any combination of the fused operands a network conv carries (test aid for those paths of every conv
 * kernel; dtype, stride, act, slope, impl and sums_dev as in the entry points above, impl = 0 for MI355_F16):
 *   x1_dev != NULL: virtual concat cat(x0, x1) along channels, x0 [n,d,h,w,c0] first, x1 [n,d,h,w,c1] (plain NDHWC of dtype),
 *     read as two tensors and never concatenated; weight_host [cout][c0 + c1][3][3][3];
 *   in_scale_dev / in_shift_dev != NULL (device fp32 [n][c0]): x0 is a producer's raw output, normalised while staging as
 *     x0 * in_scale + in_shift, then LeakyReLU(slope) when in_act = 1, BEFORE the zero padding;
 *   head_out_dev != NULL: fused 1x1x1 head, head_out [n][head_ncls][Vo] fp32 = head_w [head_ncls][cout] . act(conv) + head_b
 *     (device fp32); the feature map is not stored and y_dev must be NULL.  Otherwise y_dev receives it (plain NDHWC).
 * Combinations go to the kernel dispatchers unchanged: whatever they cannot run is refused (MI355_ERR_*, mi355_last_error). */
int mi355_conv3d_fused_ndhwc(const void *x0_dev, const void *x1_dev, int dtype, int n, int d, int h, int w, int c0, int c1,
                             const float *weight_host, const float *bias_host, int cout, int stride, int act, float slope,
                             int impl, const float *in_scale_dev, const float *in_shift_dev, int in_act,
                             const float *head_w_dev, const float *head_b_dev, int head_ncls, float *head_out_dev,
                             void *y_dev, double *sums_dev, void *stream);
/* Dry run of mi355_conv3d_fused_ndhwc (test aid; needs no device and launches nothing): which kernel instantiation a call of
 * this shape is dispatched to, with which grid, dynamic LDS size, split-K slice count and output tile - computed by the same pack
 * layout and planner code a real call runs, the single-op first-layer shortcut (c0 + c1 = 4) included.  has_stats / has_in_norm:
 * sums_dev / in_scale_dev would be non-NULL; head_ncls > 0: the fused head with that many classes.  A call the dispatch refuses
 * returns its error code (also in out->rc) and leaves the reason in mi355_last_error.  For the first-layer and the direct
 * (impl = 1) kernel only the name is filled.  No reference counterpart. */
typedef struct mi355_conv_plan {
    int32_t rc;
    char kernel[96];  /* as mi355_last_conv_kernel */
    int32_t grid[3];  /* x, y, z */
    int64_t lds_bytes;
    int32_t splitk;   /* slices of a split-K launch, 1 = none */
    int32_t tile[3];  /* output tile z, y, x */
    int32_t fuses_in_norm;  /* 1: the network would leave the producer's normalisation to this conv (asked without has_in_norm) */
} mi355_conv_plan;
int mi355_conv3d_plan(int dtype, int n, int d, int h, int w, int c0, int c1, int cout, int stride, int impl, int has_stats,
                      int has_in_norm, int head_ncls, mi355_conv_plan *out);
/* The same for a call that carries the least-padding hint of the stride-2 LDS-DMA planner (s2_least_padding != 0; MI355_S2_LEAST_PADDING,
 * csrc/kernels.h ConvCall::s2_least_padding): where conv3_f32_s2dma_kernel takes the call, the tile shape - 2 x 2 x 32 or 2 x 4 x 16 -
 * whose padded output columns times padded rows are fewer, ties to 2 x 2 x 32.  Only enc[1][0] of the shared level 1 sets the hint;
 * with s2_least_padding = 0 this is mi355_conv3d_plan. */
int mi355_conv3d_plan_hinted(int dtype, int n, int d, int h, int w, int c0, int c1, int cout, int stride, int impl, int has_stats,
                             int has_in_norm, int head_ncls, int s2_least_padding, mi355_conv_plan *out);
/* The kernel instantiations the 3x3x3 conv dispatch can launch (test aid; needs no device and launches nothing): one
 * "table | name\n" line per row of the four row tables (f32_rows, wino3_rows, f16_rows, s2h_rows), name as mi355_conv3d_plan and
 * mi355_last_conv_kernel spell it (without the " split-K" suffix).  Writes at most buf_bytes bytes, NUL-terminated, and returns
 * the bytes the whole list needs (buf may be NULL when buf_bytes is 0).  No reference counterpart. */
int64_t mi355_conv_kernel_names(char *buf, int64_t buf_bytes);
/* Dry run of mi355_tconv3d_ndhwc / mi355_tconv3d_ndhwc_f16 (test aid; needs no device and launches nothing): the transposed-conv
 * kernel a call of this shape is sent to, by the planner a real call and the network run.  Fills rc, kernel, grid and lds_bytes
 * (the kernel's static LDS); splitk stays 1, tile and fuses_in_norm 0.  A shape the kernels do not take (cin, cout, 2^30 voxels
 * or more) returns its error code (also in out->rc) and leaves the launcher's message in mi355_last_error.  No reference
 * counterpart. */
int mi355_tconv3d_plan(int dtype, int n, int d, int h, int w, int cin, int cout, mi355_conv_plan *out);
/* Dry run of the shared stage 0 of the sliding window (needs no device and launches nothing; the same code mi355_sw_predict /
 * mi355_sw_partial[_folds] run).  An fp32 network whose encoder stage 0 is r stride-1 blocks without run-time statistics
 * (BatchNorm folded or no norm) computes that stage once per mirror over the whole padded volume, and per (tile, mirror) over
 * one thin input slab at every tile face that lies inside the volume; the tile's level-0 features are gathered from the two
 * (a voxel within r of such a face from that face's slab - first flagged face in the order below -, every other voxel from
 * the whole-volume result).  Geometry is given in the coordinates of the (mirrored) pass: the padded volume flipped along the
 * axes of the mirror mask, where a tile's origin along a flipped axis is padded - patch - origin.
 * mirror_axes as mi355_sw_opts; r = 0 stands for a network that does not qualify.  `shared` = 0 (one tile, r = 0, or a patch
 * thinner than a slab): every tile runs stage 0 itself, as with MI355_SHARE_STAGE0=0 (the switch itself is not consulted here).
 * Returns the number of (tile, mirror) samples, tile-major, written to samples[] (at most max_samples; samples may be NULL),
 * or a negative error code.  No reference counterpart. */
typedef struct mi355_stage0_geom {
    int32_t shared;
    int32_t r;
    int32_t n_tiles, n_mirrors;
    int32_t padded[3];          /* the volume padded to at least one patch (z, y, x) */
    int32_t volume[3];          /* the whole-volume pass: padded[] zero-extended to whole 4 x 8 x 8 conv tiles */
    int32_t slab_thickness[3];  /* along the face's axis */
} mi355_stage0_geom;
typedef struct mi355_stage0_sample {
    int32_t tile, mirror;        /* tile index (z outer .. x inner); mirror mask: bit0 flips z, bit1 y, bit2 x */
    int32_t origin[3];           /* of the tile, in its pass */
    int32_t face[6];             /* z lo, z hi, y lo, y hi, x lo, x hi: 1 = the face lies inside the volume and gets a slab */
    int32_t slab_origin[6][3];   /* of the face's slab, in its pass (zeros for an unflagged face) */
    int32_t slab_shape[6][3];
} mi355_stage0_sample;
int mi355_stage0_plan(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes, int r,
                      mi355_stage0_geom *out, mi355_stage0_sample *samples, int max_samples);
/* Dry run of the shared skip half (needs no device and launches nothing; the decision code mi355_sw_predict /
 * mi355_sw_partial[_folds] run).  The first block of the last decoder stage reads the concat (upsampled, skip) and is linear in
 * front of its bias and activation; where its skip is the output of a shared stage 0, the skip half of that conv is one more
 * layer of the shared pass - computed once per mirror over the whole volume and over the slabs, whose chain is then r + 1 deep -
 * and every tile runs the upsampled half alone, adding the gathered skip half in its epilogue.  On when: fp32; the shared stage 0
 * is on (r >= 1, more than one tile, patch >= slab of the deeper chain); the block has stride 1, no run-time norm and no unfolded
 * BatchNorm; its skip is enc[0]'s output; the stage has a second block (head_ncls = 0); one sample of the patch shape with c_up channels goes to conv3_f32_wino3_kernel<0, false>
 * (whose twin with the addend epilogue, <3, false>, then runs it);
 * and MI355_SHARE_SKIP_CONV is not 0.  batch_tiles, rank and world are accepted and, by construction, not consulted: every rank
 * and lane computes a tile the same way.  No reference counterpart. */
typedef struct mi355_skip_share_net {
    int32_t dtype;          /* MI355_F32 / MI355_F16 */
    int32_t norm;           /* MI355_NORM_* of the network */
    int32_t nonlin_first;
    int32_t enc0_blocks;    /* blocks of encoder stage 0 */
    int32_t stride;         /* of the last decoder stage's first block */
    int32_t skip_is_enc0;
    int32_t c_up, c_skip, cout;
    int32_t head_ncls;      /* > 0: that block is the stage's only one - the network's last conv, which may carry the fused head */
} mi355_skip_share_net;
typedef struct mi355_skip_share_geom {
    int32_t stage0_shared, skip_shared;
    int32_t r;                  /* shell depth of the skip (stage-0 blocks) */
    int32_t skip_shell;         /* shell depth of the skip half: r + 1, or 0 when off */
    int32_t n_tiles, n_mirrors;
    int32_t volume[3];
    int32_t slab_thickness[3];  /* smallest multiple of (4, 8, 8) >= 2 (r + 1) when on, >= 2 r otherwise */
} mi355_skip_share_geom;
int mi355_skip_share_plan(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes,
                          const mi355_skip_share_net *net, int batch_tiles, int rank, int world, mi355_skip_share_geom *out);
/* One stride-1 conv on conv3_f32_wino3_kernel<0, false> - with an addend its twin <3, false> - whatever the size (test aid: the dispatch sends launches of a few tiles
 * elsewhere): y = act(bias + conv(cat(x0, x1)) + addend), x1_dev / addend_dev may be NULL; d % 4 == h % 8 == w % 8 == 0,
 * c0 % 16 == c1 % 16 == 0, cout % 32 == 0; addend_dev [n,d,h,w,cout].  Refused (MI355_ERR_UNSUPPORTED) otherwise. */
int mi355_conv3d_wino3_ndhwc(const float *x0_dev, const float *x1_dev, int n, int d, int h, int w, int c0, int c1,
                             const float *weight_host, const float *bias_host, int cout, int act, float slope,
                             const float *addend_dev, float *y_dev, void *stream);
/* ---- stage-0 views (MI355_STAGE0_VIEWS; csrc/sliding_window.hip "stage-0 views").  With the shared stage 0 and the shared skip half on, the
 * two tile tensors a forward gathers - the level-0 features and the skip half S - differ from the whole-volume tensors only inside
 * the shells (within r, for S r + 1, voxels of a tile face that lies inside the volume), and each has one reader: the first
 * stride-2 conv, the addend epilogue of the up-half launch.  Where the reader can, it reads the whole-volume tensor in place
 * through a per-sample view and only shell voxels from the tile tensor, and the gather writes the shells alone.  Results are
 * bit-identical either way. ---- */
/* Dry run (needs no device and launches nothing; the decision code mi355_sw_predict / mi355_sw_partial[_folds] run).  net as for
 * mi355_skip_share_plan; c_level1 = output channels of the first block of level 1 (c_skip -> c_level1, stride 2); batch_samples =
 * (tile, mirror) samples per forward, 0 = a full batch of one rank with batch_tiles = 0 (the same helper sizes the real call's
 * batches); the real call decides per forward, so a short last batch, or the share of the tiles one rank of several gets, is
 * asked for with its own sample count.  half_viewed: the shared skip half is on; enc0_viewed: also, a forward
 * of that many samples sends that block to conv3_f32_s2dma_kernel.  Returns the number of (tile, mirror) samples, tile-major as
 * mi355_stage0_plan lists them, written to samples[] (at most max_samples; may be NULL), or a negative error code. */
typedef struct mi355_stage0_view_geom {
    int32_t enc0_viewed, half_viewed;
    int32_t depth[2];           /* shell depth of the level-0 features (r) and of S (r + 1, 0 when the skip half is not shared) */
    int32_t n_tiles, n_mirrors;
    int32_t volume[3];          /* of one whole-volume result */
} mi355_stage0_view_geom;
typedef struct mi355_stage0_view_sample {
    int64_t offset;             /* of the tile's origin voxel in the whole-volume tensor, in voxels: (mirror index * volume + origin) */
    int32_t faces;              /* bit f: face f (z lo, z hi, y lo, y hi, x lo, x hi) lies inside the volume */
    int32_t pad_;
    int64_t shell_voxels[2];    /* voxels of the tile the gather still writes, per tensor */
} mi355_stage0_view_sample;
int mi355_stage0_view_plan(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes,
                           const mi355_skip_share_net *net, int c_level1, int batch_samples, mi355_stage0_view_geom *out,
                           mi355_stage0_view_sample *samples, int max_samples);
/* A view as the single-op entries below take it: sample i of the call is the box at samples[i].origin of volume samples[i].wv of
 * src_dev [n_wv][volume][channels] (channels = those of the tensor the view stands in for); a voxel within `depth` of a face whose
 * bit is set in samples[i].faces is read from the dense tensor, every other voxel from src_dev.  Refused (MI355_ERR_INVALID,
 * nothing is launched): a sample that leaves its tensor, n_samples other than the call's, a shell deeper than half a tile. */
typedef struct mi355_stage0_view {
    const float *src_dev;
    int32_t n_wv, volume[3], depth, n_samples;
    struct {
        int32_t wv;
        int32_t origin[3];
        int32_t faces;
    } samples[64];
} mi355_stage0_view;
/* One stride-2 conv on conv3_f32_s2dma_kernel - with a view its twin conv3_f32_s2dma_kernel_view - (test aid; force: also below
 * the size the dispatch sends there): y = act(bias + conv(x)), x_dev [n,d,h,w,cin] the dense tile tensor, cin % 8 == 0,
 * cout % 64 == 0.  Refused (MI355_ERR_UNSUPPORTED) where the kernel does not take the shape. */
int mi355_conv3d_s2dma_view_ndhwc(const float *x_dev, const mi355_stage0_view *view, int n, int d, int h, int w, int cin,
                                  const float *weight_host, const float *bias_host, int cout, int act, float slope, int force,
                                  float *y_dev, void *stream);
/* The same with the least-padding hint (mi355_conv3d_plan_hinted) on the call; s2_least_padding = 0: mi355_conv3d_s2dma_view_ndhwc. */
int mi355_conv3d_s2dma_hinted_ndhwc(const float *x_dev, const mi355_stage0_view *view, int n, int d, int h, int w, int cin,
                                    const float *weight_host, const float *bias_host, int cout, int act, float slope, int force,
                                    int s2_least_padding, float *y_dev, void *stream);
/* mi355_conv3d_s2dma_hinted_ndhwc without a view over a virtual concat [x0 | x1]: x0_dev [n,d,h,w,c0], x1_dev [n,d,h,w,c1], c0 and c1
 * multiples of 8, weight_host [cout][c0 + c1][27] (test aid: the channel chunks the kernel fetches from the second tensor). */
int mi355_conv3d_s2dma_concat_ndhwc(const float *x0_dev, const float *x1_dev, int n, int d, int h, int w, int c0, int c1,
                                    const float *weight_host, const float *bias_host, int cout, int act, float slope, int force,
                                    int s2_least_padding, float *y_dev, void *stream);
/* The second weight pack of an fp32 stride-2 layer (test aid; needs no device): every weight cut into three bf16 pieces, hi + mid + lo
 * = the weight exactly, in the order the lanes of conv3_f32_s2dma_kernel read them (layout: pack_conv_weights_s2split in conv3d.hip).
 * weight_host [cout][cin][27]; cin_pad a multiple of 8, cout of 64.  Returns the pack's length in 16-bit elements
 * (cout/64 * cin_pad/8 * 3 * 13824) and fills `out` when out_elems is at least that; negative on a bad argument. */
int64_t mi355_conv_s2_split_pack(const float *weight_host, int cin, int cin_pad, int cout, uint16_t *out, int64_t out_elems);
/* mi355_conv3d_wino3_ndhwc with an addend (conv3_f32_wino3_kernel<3, false>) that is read through a view: addend_dev [n,d,h,w,cout]
 * the dense tile tensor; view (channels = cout) may be NULL. */
int mi355_conv3d_wino3_view_ndhwc(const float *x0_dev, int n, int d, int h, int w, int c0, const float *weight_host,
                                  const float *bias_host, int cout, int act, float slope, const float *addend_dev,
                                  const mi355_stage0_view *view, float *y_dev, void *stream);
/* ---- the kernels around the convolutions, one launch each (test aids; no reference counterpart beyond the one named at the
 * kernel in csrc/elementwise.hip, stage0_gather.hip or aggregate.hip).  Each call runs the launcher the network runs and waits for `stream`.  Tensors are taken in
 * the layout the network holds them in: fp32 plain NDHWC ([N][V][C]), fp16 channel-blocked ([N][C / 8][V][8]), AS IS. ---- */
/* stats_dev [n][c][2] fp64 (sum, sum of squares over `count` voxels) -> scale_dev / shift_dev [n][c] fp32 with
 * norm(x) = x * scale + shift: biased variance (clamped at 0), eps inside the root.  kind = MI355_NORM_INSTANCE, or
 * MI355_NORM_GROUP with `groups` groups of c / groups consecutive channels (c % groups != 0 is refused).  gamma_dev / beta_dev
 * [c] fp32 or NULL (1 / 0). */
int mi355_norm_finalize(const double *stats_dev, int n, int c, int64_t count, int kind, int groups, float eps,
                        const float *gamma_dev, const float *beta_dev, float *scale_dev, float *shift_dev, void *stream);
/* In place: x = act(x * scale[n][c] + shift[n][c]) over n samples of v voxels; act 1 = LeakyReLU(slope).  c % 4 == 0 (fp32),
 * c % 8 == 0 (fp16). */
int mi355_norm_apply(void *x_dev, int dtype, int n, int64_t v, int c, const float *scale_dev, const float *shift_dev, int act,
                     float slope, void *stream);
/* vol_dev [c][z][y][x] fp32 sits at offset pad[] (z, y, x) in a zero volume; sample i is the patch[]-sized box at
 * tiles_host[4 i .. 4 i + 2] (z, y, x) of that volume, flipped along the axes of the mask tiles_host[4 i + 3] (bit0 z, bit1 y,
 * bit2 x), written to x_dev [n_samples][patch voxels][cpad] of dtype (fp16 with cpad % 8 == 0: channel-blocked); channels
 * >= c are zero.  At most 64 samples. */
int mi355_extract_tiles(const float *vol_dev, int c, int z, int y, int x, const int32_t pad[3], const int32_t *tiles_host,
                        int n_samples, const int32_t patch[3], int cpad, void *x_dev, int dtype, void *stream);
/* 1x1x1 head: feat_dev [n][v][cin] of dtype -> logits_dev [n][ncls][v] fp32, weight_host [ncls][cin], bias_host [ncls] or NULL
 * (uploaded inside the call; cin % 8 == 0, ncls <= 8).  scale_dev / shift_dev [n][cin] fp32 or both NULL: the features are a
 * conv's raw output and the head reads max(y, slope * y) of y = x * scale + shift (slope 1: no activation). */
int mi355_head_logits(const void *feat_dev, int dtype, int n, int64_t v, int cin, const float *weight_host, const float *bias_host,
                      int ncls, const float *scale_dev, const float *shift_dev, float slope, float *logits_dev, void *stream);
/* One tile of the sliding window: samples first_sample .. first_sample + n_mirrors - 1 of feat_dev are the forwards of the
 * tile flipped by mirrors_host[] (masks as above); result = sum over them, in list order, of (1 / n_mirrors) *
 * flip_back(nonlin(head(features))); agg_dev [ncls][padded] += result * gauss_dev [patch] (NULL: 1) at origin[], cnt_dev
 * [padded] += gauss (cnt_dev may be NULL).  scale_dev / shift_dev are indexed by the sample as feat_dev is.  A tile that
 * leaves the padded grid is refused. */
int mi355_head_aggregate(const void *feat_dev, int dtype, int cin, const float *weight_host, const float *bias_host, int ncls,
                         const float *scale_dev, const float *shift_dev, float slope, int first_sample, const int32_t *mirrors_host,
                         int n_mirrors, const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *cnt_dev,
                         const int32_t padded[3], const int32_t origin[3], void *stream);
/* The same from logits_dev [samples][ncls][patch voxels] fp32 (a last conv with the fused head). */
int mi355_logits_aggregate(const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host, int n_mirrors,
                           const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *cnt_dev,
                           const int32_t padded[3], const int32_t origin[3], void *stream);
/* The same for the n_tiles tiles of one forward in one launch (per 64 tiles): tile i's samples are first_sample + i * n_mirrors ..
 * of logits_dev, its origin origins[3 i .. 3 i + 2].  Every voxel of agg_dev / cnt_dev that a tile covers is read once, receives the
 * covering tiles' terms in list order and is written once: bit-identical to mi355_logits_aggregate called tile by tile in that
 * order.  A voxel no tile covers is not written. */
int mi355_logits_aggregate_tiles(const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host, int n_mirrors,
                                 const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *cnt_dev,
                                 const int32_t padded[3], const int32_t *origins, int n_tiles, void *stream);
/* The three above with the second moment kept (the fold mean of run_brats2021_inference_singlethread.py:97-128 extended by its
 * spread): agg2_dev [ncls][padded] += (sum over the mirrors of (1 / n_mirrors) * p^2) * gauss, read and written as agg_dev is;
 * agg_dev and cnt_dev come out bit-identical to the plain call.  nonlin = identity is refused. */
int mi355_head_aggregate_m2(const void *feat_dev, int dtype, int cin, const float *weight_host, const float *bias_host, int ncls,
                            const float *scale_dev, const float *shift_dev, float slope, int first_sample, const int32_t *mirrors_host,
                            int n_mirrors, const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *agg2_dev,
                            float *cnt_dev, const int32_t padded[3], const int32_t origin[3], void *stream);
int mi355_logits_aggregate_m2(const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host, int n_mirrors,
                              const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *agg2_dev, float *cnt_dev,
                              const int32_t padded[3], const int32_t origin[3], void *stream);
int mi355_logits_aggregate_tiles_m2(const float *logits_dev, int ncls, int first_sample, const int32_t *mirrors_host, int n_mirrors,
                                    const int32_t patch[3], int nonlin, const float *gauss_dev, float *agg_dev, float *agg2_dev,
                                    float *cnt_dev, const int32_t padded[3], const int32_t *origins, int n_tiles, void *stream);
/* cnt_dev [padded] += gauss_dev [patch] (NULL: 1) at origin[]: the normaliser of a tile another rank evaluates. */
int mi355_cnt_add_tile(const float *gauss_dev, const int32_t patch[3], float *cnt_dev, const int32_t padded[3],
                       const int32_t origin[3], void *stream);
/* The gather of the shared stage 0 (mi355_stage0_plan): out_dev [n_samples][patch][channels] fp32 from the whole-volume results
 * wv_dev [mirrors][volume][channels] and, per axis a, the slab results slab_dev[a] [slabs][S][channels] with S[a] =
 * slab_thickness[a], S[k] = patch[k] otherwise.  Sample i is the box at samples[i].origin of whole-volume result samples[i].wv;
 * slab[f] (faces z lo, z hi, y lo, y hi, x lo, x hi) = index of that face's slab in its axis's tensor, or -1: a voxel within r
 * of a face with a slab comes from that slab (the first such face in that order), every other voxel from the whole volume.
 * A hi-face slab covers the last slab_thickness layers of the tile.  Refused: a sample that leaves the volume,
 * slab_thickness < 2 r, patch < slab_thickness, channels % 4 != 0, more than 64 samples. */
typedef struct mi355_stage0_gather_args {
    const float *wv_dev;
    const float *slab_dev[3];
    float *out_dev;
    int32_t patch[3], volume[3], slab_thickness[3];
    int32_t r, channels, n_samples;
    struct {
        int32_t wv;
        int32_t origin[3];
        int32_t slab[6];
    } samples[64];
} mi355_stage0_gather_args;
int mi355_stage0_gather(const mi355_stage0_gather_args *args, void *stream);
/* The same for a tensor whose reader takes a stage-0 view: only the voxels within r of a face with a slab are written (from that
 * slab, same precedence); every other element of out_dev is left as it is. */
int mi355_stage0_gather_shells(const mi355_stage0_gather_args *args, void *stream);
/* ---- merged slabs (MI355_MERGE_SLABS, default on; csrc/sliding_window.hip "merged slabs").  Tiles that share a cut plane compute nearly the
 * same y- and x-slabs of the shared stage 0.  The gather's precedence (z shell, then y, then x) decides which padding a slab must
 * reproduce: z-slabs stay per tile; a y-slab serves only voxels outside the z shells, so it spans the extended volume in z and keeps
 * the tile's x padding - one per (mirror, side, y, x origin), box volume[0] x thickness[1] x patch[2]; an x-slab serves voxels in
 * neither other shell - one per (mirror, side, x), box volume[0] x volume[1] x thickness[2].  All keys are computed once per volume
 * behind the whole-volume pass, on every rank. ---- */
/* Dry run (no device).  r = blocks of encoder stage 0, skip_half != 0: the slab chain is one conv deeper (shared skip half).
 * Returns the number of (tile, mirror) samples, tile-major, written to samples[] (at most max_samples); slabs[] receives the
 * merged slabs, the y-slabs then the x-slabs, each list sorted by (mirror index, side, origin): n_slabs[1] + n_slabs[2] entries. */
typedef struct mi355_stage0_merge_geom {
    int32_t shared;
    int32_t r, rs;               /* shell depth of the level-0 features, and of the slab chain (r + 1 with the skip half) */
    int32_t n_tiles, n_mirrors;
    int32_t padded[3], volume[3], slab_thickness[3];
    int32_t n_slabs[3];          /* z: one per interior z face of every sample; y, x: keys */
    int32_t slab_shape[3][3];
    int64_t voxels[3];           /* n_slabs x box, per axis */
    int64_t voxels_per_tile;     /* what per-tile slabs on all three axes hold (MI355_MERGE_SLABS=0) */
} mi355_stage0_merge_geom;
typedef struct mi355_stage0_merge_slab {
    int32_t axis, mirror, side;  /* 1 = y, 2 = x; mirror mask of its pass; 0 = serves lo faces, 1 = hi faces */
    int32_t origin[3];           /* of the box, in its pass */
} mi355_stage0_merge_slab;
typedef struct mi355_stage0_merge_sample {
    int32_t tile, mirror;
    int32_t origin[3];
    int32_t slab[6];             /* z faces: 0 = the face gets a per-tile slab; y, x faces: index in that axis's list; -1: a volume face */
    int32_t offset[6][3];        /* y, x faces: where the tile's part of the slab (for a hi face its last thickness layers) starts in the slab */
} mi355_stage0_merge_sample;
int mi355_stage0_merge_plan(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes, int r, int skip_half,
                            mi355_stage0_merge_geom *out, mi355_stage0_merge_slab *slabs, int max_slabs,
                            mi355_stage0_merge_sample *samples, int max_samples);
/* mi355_stage0_gather / mi355_stage0_gather_shells (shells_only != 0) in their general form: the slabs of axis a are
 * slab_shape[a] voxels each - base.slab_thickness[a] along a; along k != a either patch[k], the tile starting at 0 (spans_volume[a][k]
 * = 0), or volume[k], the tile starting at its origin[k] (spans_volume[a][k] = 1).  An optional second tensor (out2_dev != NULL)
 * is gathered for the same samples and slab indices from its own sources, r2 >= r layers deep.  Anything else is refused. */
typedef struct mi355_stage0_gather_merged_args {
    mi355_stage0_gather_args base;
    int32_t slab_shape[3][3], spans_volume[3][3];
    const float *wv2_dev;
    const float *slab2_dev[3];
    float *out2_dev;
    int32_t r2, channels2;
} mi355_stage0_gather_merged_args;
int mi355_stage0_gather_merged(const mi355_stage0_gather_merged_args *args, int shells_only, void *stream);
/* The same for SUB-BOXES (shared level 1): sample i is the base.patch-sized box at sub[i] of a tile of `tile` voxels, origin[] its
 * own origin in the volume; a slab that does not span the volume along k holds the TILE's extent there (slab_shape[a][k] = tile[k])
 * and the box starts at sub[i][k] in it.  A face of a box that takes a shell must be a face of its tile.  by_box != 0: the launch of
 * MI355_SUBBOX_GATHER - a dense gather of one tensor runs over the boxes (stage0_gather_box_kernel) instead of over the whole
 * volume's rows; the same bytes.  (The shells-only form has one launch form.) */
typedef struct mi355_stage0_gather_boxes_args {
    mi355_stage0_gather_merged_args merged;
    int32_t tile[3];
    int32_t sub[64][3];
} mi355_stage0_gather_boxes_args;
int mi355_stage0_gather_boxes(const mi355_stage0_gather_boxes_args *args, int shells_only, int by_box, void *stream);
/* ---- shared level 1 (MI355_SHARE_LEVEL1: 0 off, unset the default rule, 2 wherever possible; csrc/sliding_window.hip "shared
 * level 1"): the geometry and the decision mi355_sw_predict / mi355_sw_partial[_folds] run, as a dry run (no device; nothing is
 * launched).  A stride-2 conv commutes with shifts by an even number of voxels, so along
 * an axis on which every (tile, mirror) sample starts at an even voxel, encoder level 1 and the skip half of the conv that reads
 * its output can be computed once per REGION - patch[a] on a per-origin axis, the whole extended volume on a merged one - and, per
 * tile face that lies inside the region on a merged axis, over one thin level-1 SLAB cut from the 2 slab_thickness outermost
 * level-0 layers of the tile; a tile's level-1 tensors are then the region's, with shells of depth d1 (enc[1]'s output) and dS
 * (the skip half) from the slabs, z before y before x.
 * On when: the shared stage 0, the shared skip half and the stage-0 views are on; encoder stage 1 and the first block of decoder
 * stage num_pool - 2 carry no run-time statistics; that stage has a second block and reads encoder stage 1's output; one sample of
 * the half patch with c_up1 channels goes to conv3_f32_wino3_kernel<3, false>; the regions' first conv goes to
 * conv3_f32_s2dma_kernel; at least one axis is merged and patch / 2 >= 2 slab_thickness on each.
 * net: the last decoder stage as mi355_skip_share_plan takes it, then level 1.  mode: 0 off, 1 the default rule (also patch / 2 >=
 * 8 slab_thickness on every merged axis, and a region that is a whole number of 4 x 8 x 8 conv tiles at level 1), 2 wherever it
 * is possible.  (The switch is also read at mi355_unet_create: at 0 the weight packs of the two halves are not made and the net never
 * takes the path.  While the path is on a forward holds at most 32 samples; a larger batch_tiles is split, which
 * mi355_stage0_view_plan, asked for more samples than that, does not know.)  Returns the number of samples, tile-major as
 * mi355_stage0_plan lists them (0 when not possible), or a negative error code.  Takes no batch, rank or world: the plan depends
 * on the network and the geometry of all tiles only. */
typedef struct mi355_level1_share_net {
    mi355_skip_share_net last;
    int32_t num_pool;
    int32_t enc1_blocks;         /* blocks of encoder stage 1: one stride-2 block, then stride-1 blocks */
    int32_t c_level1;            /* their output channels */
    int32_t skip_is_enc1;        /* the second input of the first block of decoder stage num_pool - 2 is encoder stage 1's output */
    int32_t dec1_blocks;         /* blocks of that decoder stage */
    int32_t c_up1, cout1;        /* of its first block: channels of the upsampled half, output channels */
} mi355_level1_share_net;
typedef struct mi355_level1_share_geom {
    int32_t possible, on;        /* the geometry allows it; the decision under `mode` */
    int32_t r0, k1, d1, dS;      /* blocks of stage 0 and of stage 1; shell depths at level 1 */
    int32_t n_tiles, n_mirrors, n_regions;
    int32_t padded[3], volume[3];
    int32_t stage0_slab_thickness[3];  /* of the stage-0 slabs that give a region its level-0 shells */
    int32_t merged[3];
    int32_t region[3];           /* level-0 extent of a region */
    int32_t slab_thickness[3];   /* level 1; 0 on a per-origin axis */
    int32_t n_slabs[3];
    int64_t region_voxels, slab_voxels, tile_voxels;  /* level-1 voxels: all regions, all slabs, all samples (the per-tile count) */
} mi355_level1_share_geom;
typedef struct mi355_level1_share_region {
    int32_t mirror;              /* mask of its pass */
    int32_t origin[3];           /* in that pass; 0 on a merged axis */
    int32_t faces;               /* bit f: face f lies inside the volume on a per-origin axis and takes stage-0 shells */
} mi355_level1_share_region;
typedef struct mi355_level1_share_sample {
    int32_t tile, mirror, region;
    int32_t origin[3];           /* of the tile in its pass */
    int32_t origin1[3];          /* of the tile inside its region, at level 1 */
    int32_t faces;               /* bit f: tile face f lies inside the volume */
    int32_t slab[6];             /* 1: face f has a level-1 slab */
    int32_t slab_offset[6][3], slab_shape[6][3];  /* the level-0 sub-box of the tile the slab is cut from */
} mi355_level1_share_sample;
int mi355_level1_share_plan(int z, int y, int x, const int32_t patch[3], double step_size, int mirror_axes,
                            const mi355_level1_share_net *net, int mode, mi355_level1_share_geom *out,
                            mi355_level1_share_region *regions, int max_regions, mi355_level1_share_sample *samples, int max_samples);
/* x_dev [n][volume][c] fp32: zero every voxel outside [0, keep) (c % 4 == 0, 0 < keep <= volume); the rest is not written. */
int mi355_stage0_mask(float *x_dev, int n, const int32_t volume[3], const int32_t keep[3], int c, void *stream);
/* Name of the kernel instantiation the calling thread's last mi355_conv3d_ndhwc / mi355_conv3d_ndhwc_f16 call dispatched
 * (the names rocprofv3 and mi355_profile_read show).  Test aid: a parity case written for one kernel can assert that it
 * ran on that kernel.  No reference counterpart (torch.nn.Conv3d, generic_UNet.py:56, has one implementation). */
const char *mi355_last_conv_kernel(void);

#ifdef __cplusplus
}
#endif
#endif /* MI355_NNUNET_H */
