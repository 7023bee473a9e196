"""ctypes binding of libwesup_hip.so (C ABI in include/wesup_hip.h).

The product path has NO CPU fallback: if the shared library is missing or a
kernel entry fails, this module raises.  ``build()`` compiles it with hipcc for
gfx950 (cross-compiles without a GPU).
"""
import ctypes
import functools
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
# WESUP_HIP_LIB: another build of the same library (A/B measurements of kernel variants in one GPU session)
LIB_PATH = os.environ.get('WESUP_HIP_LIB') or os.path.join(CSRC, 'libwesup_hip.so')

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_float = ctypes.c_float
c_size_t = ctypes.c_size_t

# name -> (restype, [argtypes]);  'p' pointer, 'i' int, 'f' float, 'z' size_t, 'l' long
_SIGS = {
    'wesup_abi_version': (c_int, ''),
    'wesup_debug_clock': (c_int, 'p'),
    'wesup_debug_set_trace': (c_int, 'p'),
    'wesup_strerror': (ctypes.c_char_p, 'i'),
    'wesup_augment': (c_int, 'pppppiiippiiiip'),
    'wesup_appearance_workspace_bytes': (c_size_t, 'iii'),
    'wesup_appearance': (c_int, 'pppiiipzp'),
    'wesup_pack_input': (c_int, 'ppiiip'),
    'wesup_conv3x3_kpad': (c_int, 'i'),
    'wesup_pack_conv3x3_weight': (c_int, 'pppiip'),
    'wesup_transpose': (c_int, 'ppiip'),
    'wesup_transpose_batched': (c_int, 'pip'),
    'wesup_scale_rows_by_area': (c_int, 'pplip'),
    'wesup_conv3x3_workspace_bytes': (c_size_t, 'iiiii'),
    'wesup_conv3x3_fwd': (c_int, 'pppppiiiiiipzp'),
    'wesup_conv3x3_fwd_side': (c_int, 'ppppppppiiiiiiip'),
    'wesup_conv3x3_dgrad': (c_int, 'ppppiiiiiipzp'),
    'wesup_conv3x3_wgrad_workspace_bytes': (c_size_t, 'iiiii'),
    'wesup_conv3x3_wgrad': (c_int, 'ppppiiiiiipzp'),
    'wesup_conv3x3_wgrad_winograd_workspace_bytes': (c_size_t, 'iiiiii'),
    'wesup_conv3x3_wgrad_winograd': (c_int, 'pppppiiiiiiipzp'),
    'wesup_winograd_weight_floats': (c_size_t, 'iii'),
    'wesup_winograd_tiles': (ctypes.c_long, 'iiii'),
    'wesup_winograd_pack_weight': (c_int, 'pppiiip'),
    'wesup_winograd_pack_weights': (c_int, 'pip'),
    'wesup_conv3x3_winograd_workspace_bytes': (c_size_t, 'iiiiii'),
    'wesup_conv3x3_fwd_winograd': (c_int, 'ppppppipiiiiiiipzp'),
    'wesup_conv3x3_dgrad_winograd': (c_int, 'ppppiiiiiiipzp'),
    'wesup_conv3x3_dgrad_winograd_unpool': (c_int, 'ppppiiiiiiiipzp'),
    'wesup_winograd_output_transform_unpool': (c_int, 'plppppiiiiiiip'),
    'wesup_winograd_fused_supported': (c_int, 'iii'),
    'wesup_winograd_fused_route': (c_int, 'iiil'),
    'wesup_winograd_set_fused_min_blocks': (c_int, 'i'),
    'wesup_winograd_gemm_output_transform': (c_int, 'plpppppippiiiiiiiip'),
    'wesup_winograd_gemm_output_transform_gather': (c_int, 'plppppiipppiiiiiip'),
    'wesup_winograd_input_transform_bits': (c_int, 'pplpiiiiip'),
    'wesup_winograd_bias_rows': (ctypes.c_long, 'iiii'),
    'wesup_winograd_dual_transform': (c_int, 'ppppiiiip'),
    'wesup_winograd_dual_transform_unpool': (c_int, 'ppi' + 'ppppp' + 'iiii' + 'p'),
    'wesup_conv3x3_wgrad_winograd_pre': (c_int, 'pppipp' + 'iiiii' + 'pzp'),
    'wesup_winograd_gemm_output_transform_ex': (c_int, 'plpppppp' + 'i' + 'pppp' + 'ii' + 'ppp' + 'iiiiiii' + 'p'),
    'wesup_conv3x3_dgrad_winograd_gather': (c_int, 'ppppppppiiiiiiiipzp'),
    'wesup_winograd_input_transform': (c_int, 'ppliiiiiip'),
    'wesup_gemm_nt_batched': (c_int, 'pilpilpiliiiip'),
    'wesup_gemm_nt_batched_bias': (c_int, 'pilpilplpiliiiip'),
    'wesup_winograd_output_transform': (c_int, 'plpppppiiiiiiip'),
    'wesup_winograd_outgrad_workspace_bytes': (c_size_t, 'iiiii'),
    'wesup_winograd_outgrad_transform': (c_int, 'pppiiiiipzp'),
    'wesup_winograd_filter_grad': (c_int, 'pllippiiip'),
    'wesup_gemm_nt_workspace_bytes': (c_size_t, 'iii'),
    'wesup_gemm_nt': (c_int, 'pipippipiiiiipzp'),
    'wesup_gemm_tn_workspace_bytes': (c_size_t, 'iii'),
    'wesup_gemm_tn': (c_int, 'pipipipiiiipzp'),
    'wesup_gemm_tn_batched_workspace_bytes': (c_size_t, 'iiii'),
    'wesup_gemm_tn_batched_k_per_split': (c_int, 'iiii'),
    'wesup_gemm_tn_batched': (c_int, 'pilpilpiliiiiipzp'),
    'wesup_colsum_workspace_bytes': (c_size_t, 'ii'),
    'wesup_colsum': (c_int, 'pipiipzp'),
    'wesup_maxpool2_fwd': (c_int, 'ppiiiiip'),
    'wesup_maxpool2_bwd': (c_int, 'pppiiiiip'),
    'wesup_upsample_fwd': (c_int, 'ppiiiiiiiip'),
    'wesup_upsample_bwd': (c_int, 'ppppiiiiiiiiip'),
    'wesup_upsample_bwd_group': (c_int, 'ppppppiiiippiiiiiip'),
    'wesup_sp_preprocess_workspace_bytes': (c_size_t, 'iiii'),
    'wesup_sp_preprocess': (c_int, 'ppiiii' + 'pppppppppp' + 'ppi' + 'pzp'),
    'wesup_spmaps_to_labels': (c_int, 'ppiip'),
    'wesup_sp_max_units': (c_int, 'ii'),
    'wesup_sp_segments': (c_int, 'piiippp'),
    'wesup_sp_pool_workspace_bytes': (c_size_t, 'iii'),
    'wesup_sp_pool_fwd': (c_int, 'ppppppiiiiiipzp'),
    'wesup_sp_pool_bwd': (c_int, 'ppppiiiiip'),
    'wesup_sp_pool_upsample_fwd': (c_int, 'ppppppiiiiiiiiiipzp'),
    'wesup_sp_interp_matrix': (c_int, 'pppiiiiiip'),
    'wesup_sp_pool_mat_route': (c_int, 'ii'),
    'wesup_sp_pool_mat_fwd': (c_int, 'pppp' + 'ii' + 'iiii' + 'pzp'),
    'wesup_sp_pool_mat_bwd': (c_int, 'ppp' + 'ii' + 'p' + 'iiii' + 'pzp'),
    'wesup_paint_fwd': (c_int, 'pppiiiiip'),
    'wesup_slic_num_centers': (c_int, 'iii'),
    'wesup_slic_workspace_bytes': (c_size_t, 'iiii'),
    'wesup_slic': (c_int, 'pppiiiifiifpzp'),
    'wesup_classifier_fwd': (c_int, 'ppppiip'),
    'wesup_classifier_bwd_workspace_bytes': (c_size_t, 'ii'),
    'wesup_classifier_bwd': (c_int, 'ppppppppiipzp'),
    'wesup_propagate': (c_int, 'ppppfipppiiiip'),
    'wesup_loss_fwd': (c_int, 'ppppffppiiip'),
    'wesup_loss_bwd': (c_int, 'ppppppffpiiip'),
    'wesup_head_fwd': (c_int, 'pppppppfipppiiiip'),
    'wesup_head_bwd': (c_int, 'pppppppffpppiiiipzp'),
    'wesup_classifier_bwd_finish': (c_int, 'pzppiip'),
    # the C-way head, 2 <= C <= WESUP_MAX_CLASSES (csrc/loss.hip)
    'wesup_classifier_fwd_c': (c_int, 'ppppiiip'),
    'wesup_classifier_bwd_c_workspace_bytes': (c_size_t, 'iii'),
    'wesup_classifier_bwd_c': (c_int, 'ppppppppiiipzp'),
    'wesup_head_fwd_c': (c_int, 'pppppppfipppiiiip'),
    'wesup_head_bwd_c': (c_int, 'pppppppffpppiiiipzp'),
    'wesup_classifier_bwd_c_finish': (c_int, 'pzppiiip'),
    'wesup_paint_argmax_workspace_bytes': (c_size_t, 'ii'),
    'wesup_paint_argmax': (c_int, 'pppiiiipzp'),
    'wesup_seg_confusion': (c_int, 'ppppiiip'),
    'wesup_cross_entropy_fwd': (c_int, 'pppfpiip'),
    'wesup_cross_entropy_bwd': (c_int, 'pppppfpiip'),
    'wesup_sgd_step': (c_int, 'pppzffffip'),
    # Adam / AdamW with the step count and lr in a device block (csrc/optim.hip)
    'wesup_adam_tick': (c_int, 'pfffp'),
    'wesup_adam_step': (c_int, 'ppppzp' + 'fffffff' + 'ip'),
    'wesup_seg_metrics_workspace_bytes': (c_size_t, 'i'),
    'wesup_seg_metrics': (c_int, 'pppiiipzp'),
    # mask post-processing and challenge scoring (csrc/regions.hip)
    'wesup_cc_label_workspace_bytes': (c_size_t, 'iii'),
    'wesup_cc_label': (c_int, 'ppp' + 'iiiii' + 'pzp'),
    'wesup_remove_small_regions_workspace_bytes': (c_size_t, 'iii'),
    'wesup_remove_small_regions': (c_int, 'pp' + 'iiii' + 'pzp'),
    'wesup_binary_morph_workspace_bytes': (c_size_t, 'iiii'),
    'wesup_binary_morph': (c_int, 'ppp' + 'iiiiii' + 'pzp'),
    'wesup_contingency': (c_int, 'pppp' + 'iiii' + 'p'),
    'wesup_label_sort_workspace_bytes': (c_size_t, 'iiii'),
    'wesup_label_sort': (c_int, 'pppppp' + 'iiii' + 'pzp'),
    'wesup_directed_hausdorff_sq': (c_int, 'ppppppp' + 'iiiii' + 'p'),
    # splitting touching objects: distance map, label growth, cut (csrc/split.hip)
    'wesup_edt_sq_workspace_bytes': (c_size_t, 'iii'),
    'wesup_edt_sq': (c_int, 'pp' + 'iiii' + 'pzp'),
    'wesup_label_grow_workspace_bytes': (c_size_t, 'iii'),
    'wesup_label_grow': (c_int, 'pppp' + 'iiiiii' + 'pzp'),
    'wesup_label_cut': (c_int, 'ppp' + 'iii' + 'p'),
    # surface-distance metrics: the exact distance map, borders, the raw quantities (csrc/surface.hip)
    'wesup_edt_full_workspace_bytes': (c_size_t, 'iii'),
    'wesup_edt_full': (c_int, 'pp' + 'iiii' + 'pzp'),
    'wesup_mask_border': (c_int, 'pp' + 'iii' + 'p'),
    'wesup_surface_stats_workspace_bytes': (c_size_t, 'iii'),
    'wesup_surface_stats': (c_int, 'ppppp' + 'iii' + 'll' + 'pzp'),
    # object outlines: ordered boundary rings of a label map (csrc/contour.hip)
    'wesup_contour_workspace_bytes': (c_size_t, 'iii'),
    'wesup_contour_trace_workspace_bytes': (c_size_t, 'iiii'),
    'wesup_contour_count': (c_int, 'pp' + 'iii' + 'pzp'),
    'wesup_contour_trace': (c_int, 'ppppp' + 'iiiiii' + 'pzp'),
    # ... and their exact simplification
    'wesup_contour_simplify_workspace_bytes': (c_size_t, 'ii'),
    'wesup_contour_simplify': (c_int, 'pipii' + 'pppp' + 'pzp'),
    # object measurements: moments, shape counts, exact hulls (csrc/measure.hip)
    'wesup_measure_limit': (c_int, 'i'),
    'wesup_measure_workspace_bytes': (c_size_t, 'iiiii'),
    'wesup_measure_profile_count': (c_int, 'ppp' + 'iiii' + 'pzp'),
    'wesup_object_measure': (c_int, 'ppppp' + 'iiiiii' + 'pzp'),
    # polygon fill: fixed-point polygons in CSR form -> label maps and class maps (csrc/raster.hip)
    'wesup_raster_limit': (c_int, 'i'),
    'wesup_polygon_fill_workspace_bytes': (c_size_t, 'iiii'),
    'wesup_polygon_fill': (c_int, 'pppppppp' + 'iiiiii' + 'pzp'),
    # painted object comparisons (csrc/paint.hip)
    'wesup_object_match_workspace_bytes': (c_size_t, 'ii'),
    'wesup_object_match': (c_int, 'pppp' + 'iii' + 'pzp'),
    'wesup_label_paint': (c_int, 'pppp' + 'iii' + 'p'),
    # exact t-SNE of superpixel features (csrc/tsne.hip)
    'wesup_tsne_sqdist': (c_int, 'pii' + 'pp'),
    'wesup_tsne_affinities_workspace_bytes': (c_size_t, 'i'),
    'wesup_tsne_affinities': (c_int, 'pif' + 'pp' + 'pzp'),
    'wesup_tsne_iterate_workspace_bytes': (c_size_t, 'i'),
    'wesup_tsne_iterate': (c_int, 'ppppp' + 'ii' + 'ffff' + 'pzp'),
    # stain normalisation and stain jitter, exact order statistics (csrc/stain.hip)
    'wesup_select_f32_workspace_bytes': (c_size_t, 'l'),
    'wesup_select_f32': (c_int, 'plpip' + 'pzp'),
    'wesup_select_i32_workspace_bytes': (c_size_t, 'l'),
    'wesup_select_i32': (c_int, 'plpip' + 'pzp'),
    'wesup_stain_fit_workspace_bytes': (c_size_t, 'iiii'),
    'wesup_stain_fit_stage_offset': (c_size_t, 'iiiii'),
    'wesup_stain_fit': (c_int, 'pp' + 'iiii' + 'fffi' + 'pzp'),
    'wesup_stain_apply': (c_int, 'pppp' + 'ipf' + 'iii' + 'fp'),
    # window inference on large images (csrc/tiles.hip)
    'wesup_window_gather': (c_int, 'pppp' + 'iiiiiii' + 'p'),
    'wesup_window_merge': (c_int, 'pppp' + 'iiiiiii' + 'p'),
    # ... over windows x views: n_views and the view word, four bits per view; the two above are these at 1, 0
    'wesup_window_gather_views': (c_int, 'pppp' + 'iiiiiiiii' + 'p'),
    'wesup_window_merge_views': (c_int, 'pppp' + 'iiiiiiiii' + 'p'),
    # whole-image multi-scale pixel inference (csrc/pixel.hip)
    'wesup_image_resize_u8': (c_int, 'pp' + 'iiii' + 'p'),
    'wesup_plane_resize_acc': (c_int, 'pp' + 'iiiii' + 'fi' + 'p'),
    'wesup_pixel_gather_fwd': (c_int, 'pppp' + 'iiiii' + 'p'),
    # whole-slide evaluation: the DP2019 patch pipeline (csrc/slide.hip)
    'wesup_patch_gather_resize': (c_int, 'pp' + 'iiiiiiii' + 'p'),
    'wesup_patch_scatter_u8': (c_int, 'pp' + 'iiiiiiiii' + 'p'),
    'wesup_mask_scores': (c_int, 'ppp' + 'li' + 'p'),
    # ... over a patch list, and the tissue selection that makes one (csrc/tissue.hip)
    'wesup_patch_gather_resize_list': (c_int, 'pp' + 'iiiiiiii' + 'pi' + 'p'),
    'wesup_patch_scatter_u8_list': (c_int, 'pp' + 'iiiiiiiii' + 'pi' + 'p'),
    'wesup_patch_value_hist': (c_int, 'pp' + 'iiii' + 'p'),
    'wesup_tissue_select': (c_int, 'p' + 'iiiiii' + 'pppp' + 'p'),
    'wesup_tissue_mask_u8': (c_int, 'ppp' + 'iii' + 'p'),
    # class maps for more than two classes (csrc/classmap.hip)
    'wesup_window_merge_classes': (c_int, 'ppppp' + 'iiiiiii' + 'p'),
    'wesup_window_merge_classes_views': (c_int, 'ppppp' + 'iiiiiiiii' + 'p'),
    'wesup_planes_resize_acc': (c_int, 'pp' + 'iiiii' + 'fi' + 'p'),
    'wesup_class_argmax_u8': (c_int, 'pp' + 'li' + 'p'),
    'wesup_patch_scatter_classes_u8': (c_int, 'ppp' + 'iiiiiiiii' + 'p'),
    'wesup_patch_scatter_classes_u8_list': (c_int, 'ppp' + 'iiiiiiiii' + 'pi' + 'p'),
    'wesup_label_confusion': (c_int, 'pppp' + 'li' + 'p'),
    # weak-label preparation (csrc/prepare.hip)
    'wesup_prepare_lds_entries': (c_int, 'i'),
    'wesup_label_stats': (c_int, 'ppp' + 'iiii' + 'p'),
    'wesup_sp_vote_workspace_bytes': (c_size_t, 'iiii'),
    'wesup_sp_vote': (c_int, 'ppppp' + 'iiii' + 'pzp'),
    'wesup_spl_paint_workspace_bytes': (c_size_t, 'ii'),
    'wesup_spl_paint': (c_int, 'pppp' + 'iiiii' + 'pzp'),
    # entries by the names of SURVEY.md 8(b) (csrc/named.hip)
    'wesup_sp_stats': (c_int, 'ppiiiipppp'),
    'wesup_conv1x1_workspace_bytes': (c_size_t, 'iii'),
    'wesup_conv1x1_fwd': (c_int, 'ppppiiipzp'),
    'wesup_conv1x1_dgrad': (c_int, 'pppiiiipzp'),
    'wesup_conv1x1_wgrad': (c_int, 'ppppiiipzp'),
    'wesup_linear_workspace_bytes': (c_size_t, 'iii'),
    'wesup_linear_fwd': (c_int, 'ppppiiiipzp'),
    'wesup_linear_bwd': (c_int, 'pppppppiiipzp'),
    'wesup_upsample_bilinear_ac_fwd': (c_int, 'ppiiiiiiiip'),
    'wesup_upsample_bilinear_ac_bwd': (c_int, 'ppiiiiiiiip'),
    'wesup_softmax_ce_fwd': (c_int, 'pppfppiip'),
    'wesup_softmax_ce_bwd': (c_int, 'pppppfpiip'),
    # step plans (csrc/plan.hip)
    'wesup_plan_create': (c_int, 'p'),
    'wesup_plan_destroy': (c_int, 'p'),
    'wesup_plan_begin': (c_int, 'p'),
    'wesup_plan_end': (c_int, 'p'),
    'wesup_plan_size': (c_int, 'p'),
    'wesup_plan_kernels': (c_int, 'p'),
    'wesup_plan_replay': (c_int, 'pii'),
    'wesup_plan_diff': (c_int, 'pp'),
    'wesup_plan_node_name': (ctypes.c_char_p, 'pi'),
    'wesup_plan_node_stream': (c_void_p, 'pi'),
    'wesup_plan_node_host_ns': (c_int, 'pip'),
    'wesup_sync_slots': (c_int, ''),
    'wesup_sync_record': (c_int, 'ip'),
    'wesup_sync_wait': (c_int, 'ip'),
    'wesup_sync_synchronize': (c_int, 'i'),
    'wesup_sync_query': (c_int, 'i'),
    'wesup_copy_to_host': (c_int, 'ppzp'),
    'wesup_copy': (c_int, 'ppzp'),
    'wesup_fill_words': (c_int, 'pizp'),
}
_T = {'p': c_void_p, 'i': c_int, 'f': c_float, 'z': c_size_t, 'l': ctypes.c_long}

EXPORTS = sorted(_SIGS)
MAX_CLASSES = 16         # WESUP_MAX_CLASSES
HEAD_MAX_D = 149         # WESUP_HEAD_MAX_D: the propagation kernel's LDS tile, 1088 D + 1024 bytes, within the CU's 160 KiB
TSNE_MAX_N = 32768       # WESUP_TSNE_MAX_N: the joint probabilities are dense fp32, 4 GiB there
TSNE_MAX_D = 4096        # WESUP_TSNE_MAX_D
TSNE_STATS = 4           # WESUP_TSNE_STATS: KL, |g|, Z, sum p log p
SELECT_BLOCK = 256       # WESUP_SELECT_BLOCK
SELECT_MAX_BLOCKS = 256  # WESUP_SELECT_MAX_BLOCKS
SELECT_MAX_RANKS = 4     # WESUP_SELECT_MAX_RANKS
STAIN_BLOCK = 16         # WESUP_STAIN_BLOCK: HE[3][2], pinv[2][3], maxC[2], n_tissue, valid
SPLIT_SEG, SPLIT_ROWS = 64, 4      # WESUP_SPLIT_SEG, WESUP_SPLIT_ROWS: the distance map's row pass, 4 rows of 64 pixels per block
SPLIT_TILE, SPLIT_HALO = 32, 8     # WESUP_SPLIT_TILE, WESUP_SPLIT_HALO: the growth kernel's tile edge and halo (rounds per launch)
EDT_NONE = 2 ** 31 - 1              # WESUP_EDT_NONE: the distance map of an image without a zero pixel
EDT_CHUNK, EDT_COLS = 64, 256      # WESUP_EDT_CHUNK, WESUP_EDT_COLS: the full distance map's column pass, chunks of rows x columns per block
EDT_SEG, EDT_ROWS = 64, 4          # WESUP_EDT_SEG, WESUP_EDT_ROWS: its row pass, 4 rows of 64 pixels per block
SURFACE_STATS = 10                 # WESUP_SURFACE_STATS: 8-byte slots of a pair's block
CONTOUR_RING = 12                  # WESUP_CONTOUR_RING: int32 words of a ring record
SIMPLIFY_TOL_MAX = 4096            # WESUP_SIMPLIFY_TOL_MAX: sixteenths of a pixel
SIMPLIFY_COUNTS = 4                # WESUP_SIMPLIFY_COUNTS: kept vertices, rings flagged 1, rings flagged 2, status
MEASURE_WORDS = 24                 # WESUP_MEASURE_WORDS: int64 words of a label's row
MEASURE_HULL_CHUNK = 256           # WESUP_MEASURE_HULL_CHUNK: candidates per block of the hull test
MEASURE_LDS_LABELS = 512           # wesup_measure_limit(0): labels (L + 1) up to which a block keeps its moment table in LDS
RASTER_FRAC_BITS = 8               # WESUP_RASTER_FRAC_BITS: one pixel is 256 units
RASTER_TILE_ROWS, RASTER_TILE_COLS = 64, 64     # WESUP_RASTER_TILE_ROWS, WESUP_RASTER_TILE_COLS: the fill kernel's tile
RASTER_BLOCK = 256                 # WESUP_RASTER_BLOCK: threads that walk a feature's edges together
RASTER_COORD_MAX = 2 ** 28         # wesup_raster_limit(3): the largest |coordinate| in fixed point
TISSUE_MAX_BLOCKS = 2048           # WESUP_TISSUE_MAX_BLOCKS: the histogram kernel's grid, striding over its items
TISSUE_ITEM_PIXELS = 8192          # WESUP_TISSUE_ITEM_PIXELS: an item is max(1, this // p) rows of one patch
TISSUE_LIST_CHUNK = 256            # WESUP_TISSUE_LIST_CHUNK: patches per step of the ordered compaction
ABI_VERSION = 6          # include/wesup_hip.h; a stale libwesup_hip.so with other signatures must not be called

_lib = None


class WesupHipError(RuntimeError):
    pass


class WinoFilter(ctypes.Structure):            # WesupWinoFilter (include/wesup_hip.h)
    _fields_ = [('w', c_void_p), ('u_fwd', c_void_p), ('u_dgrad', c_void_p), ('Cout', c_int), ('Cin', c_int)]


class TransposeItem(ctypes.Structure):         # WesupTransposeItem
    _fields_ = [('src', c_void_p), ('dst', c_void_p), ('rows', c_int), ('cols', c_int)]


class CoarseMap(ctypes.Structure):             # WesupCoarseMap
    _fields_ = [('p', c_void_p), ('h', c_int), ('w', c_int)]


def build(verbose=False):
    """Compile libwesup_hip.so for gfx950 in-tree (wesup_amd/csrc)."""
    cmd = ['make', '-C', CSRC, '-j4']
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout)
    if r.returncode != 0:
        raise WesupHipError('building libwesup_hip.so failed')
    return LIB_PATH


def load():
    """Load the library (no GPU needed to load; kernels need one to run)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WesupHipError(f'{LIB_PATH} not found: run `python -c "import __graft_entry__ as g; g.build()"` '
                            '(there is no CPU fallback for the HIP path)')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = [_T[a] for a in args]
    # pure size / shape queries (integers in, an integer out): answered from a cache after the first call -- a training step asks
    # ~150 of them, the same ones every step
    for name in _SIGS:
        if name.endswith('_bytes') or name in ('wesup_winograd_tiles', 'wesup_winograd_fused_supported', 'wesup_winograd_bias_rows',
                                               'wesup_conv3x3_kpad', 'wesup_sp_max_units'):
            if all(a in 'il' for a in _SIGS[name][1]):
                setattr(lib, name, functools.lru_cache(maxsize=4096)(getattr(lib, name)))
    if lib.wesup_abi_version() != ABI_VERSION:
        raise WesupHipError(f'{LIB_PATH} has ABI version {lib.wesup_abi_version()}, this package binds version '
                            f'{ABI_VERSION}: rebuild it (make -C wesup_amd/csrc)')
    _lib = lib
    return lib


def check(rc, what=''):
    if rc != 0:
        msg = load().wesup_strerror(rc).decode()
        raise WesupHipError(f'{what} failed: {msg} (code {rc})')


def call(name, *args):
    """Call an int-returning entry and raise on a non-zero code."""
    check(getattr(load(), name)(*args), name)
