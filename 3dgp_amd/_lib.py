"""ctypes binding of libtdgp_hip.so (the C ABI declared in include/tdgp.h).

This is the "plugin loader" of the build: the counterpart of the reference's
`custom_ops.get_plugin()` (src/torch_utils/custom_ops.py:59-155), except that nothing is compiled
at run time -- the prebuilt gfx950 library is dlopen'ed.  If it is missing or fails to load the
product path raises; there is no CPU or PyTorch fallback behind these entry points.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'csrc', 'libtdgp_hip.so')     # the one library of the product; tests / tools/dev rebind this attribute before load()

P = c_void_p
_PROTOTYPES = {
    'tdgp_version': (c_int, []),
    'tdgp_last_error': (c_char_p, []),
    'tdgp_profile_enable': (c_int, [c_int]),
    'tdgp_profile_report': (c_int64, [c_char_p, c_int64]),
    'tdgp_device_fault': (c_int, [c_int]),
    'tdgp_bias_act': (c_int, [P, P, P, c_int64, c_int, c_int64, c_int, c_float, c_float, c_float, c_int, P]),
    'tdgp_bias_act_grad': (c_int, [P, P, P, P, P, P, c_int64, c_int, c_int64, c_int, c_int, c_float, c_float, c_float, c_int, P]),
    'tdgp_upfirdn2d': (c_int, [P, P, P, c_int, c_int, c_int, c_int, POINTER(c_int64), c_int, c_int, POINTER(c_int64),
                               c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, P]),
    'tdgp_modconv_pack_bytes': (c_int64, [c_int, c_int, c_int]),
    'tdgp_modconv_pack': (c_int, [P, P, c_int, c_int, c_int, P]),
    'tdgp_modconv2d_workspace_bytes': (c_int64, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'tdgp_modconv2d_takes_folded_up2': (c_int, [c_int, c_int, c_int, c_int, c_int]),
    'tdgp_modconv2d_path': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    'tdgp_conv2d': (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    'tdgp_conv2d_weight_grad_workspace_bytes': (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    'tdgp_conv2d_weight_grad': (c_int, [P, P, P, P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P]),
    'tdgp_conv_transpose2d_x2': (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, c_int, P, c_int64, P]),
    'tdgp_set_conv_arith': (c_int, [c_int]),
    'tdgp_modconv_wsq_offset': (c_int64, [c_int, c_int, c_int]),
    'tdgp_demod_batch': (c_int, [P, P, P, c_int, c_int, c_int, P]),
    'tdgp_modconv2d': (c_int, [P, P, P, P, P, c_int64, P, POINTER(c_float), P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                               c_int, c_int, c_float, c_float, c_float, c_int, c_int, P, c_int64, P]),
    'tdgp_modconv2d_bf16': (c_int, [P, P, P, P, P, c_int64, P, POINTER(c_float), P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_float, c_float, c_float, c_int, c_int, P, c_int64, P]),
    'tdgp_cast_f32_bf16': (c_int, [P, P, c_int64, P]),
    'tdgp_style_affine': (c_int, [P, P, P, P, P, P, c_int, c_int, c_int, c_int, P]),
    'tdgp_cam2world': (c_int, [P, P, P, P, c_int, P]),
    'tdgp_sample_rays': (c_int, [P, P, c_int, P, P, P, P, c_int, c_int, c_int, P]),
    'tdgp_sample_stratified': (c_int, [P, P, P, c_int64, c_int, c_int, c_float, c_float, P]),
    'tdgp_density_activation': (c_int, [P, P, c_int64, c_int, c_float, P]),
    'tdgp_planes_to_hwc': (c_int, [P, P, c_int, c_int, c_int, c_int, P]),
    'tdgp_triplane_features': (c_int, [P, P, P, c_int, c_int64, c_int, c_int, c_int, c_float, P]),
    'tdgp_triplane_field': (c_int, [P, P, P, P, P, P, P, P, P, P, c_float, P, P, c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                    c_int, P]),
    'tdgp_ray_march': (c_int, [P, P, P, P, P, P, P, c_int64, c_int, c_int, c_int, c_int, c_float, c_float, P]),
    'tdgp_triplane_field_grad_workspace_bytes': (c_int64, [c_int, c_int64, c_int, c_int]),
    'tdgp_triplane_field_grad': (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, c_int64, c_int, c_int64, c_int, c_int, c_int, c_int, c_float, c_int, P]),
    'tdgp_triplane_field_deep': (c_int, [P, P, P, P, P, P, P, c_int, P, c_float, P, P, c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                                         c_int, P]),
    'tdgp_triplane_field_deep_grad_workspace_bytes': (c_int64, [c_int, c_int64, c_int, c_int, c_int]),
    'tdgp_triplane_field_deep_grad': (c_int, [P, P, P, P, c_int, P, P, P, P, P, P, c_int64, c_int, c_int64, c_int, c_int, c_int, c_int, c_float, c_int, P]),
    'tdgp_ray_march_grad': (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int, c_int, c_int, c_int, c_float, P]),
    'tdgp_sample_importance': (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int, c_int, c_int, c_int, P]),
    'tdgp_unify_samples': (c_int, [P, P, P, c_int, P, P, P, c_int, P, P, P, P, c_int64, c_int, P]),
    'tdgp_importance_from_coarse': (c_int, [P, P, P, P, P, P, P, c_int64, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_float, P]),
    'tdgp_merge_composite': (c_int, [P, P, c_int, P, P, c_int, P, P, P, P, P, P, c_int64, c_int, c_int, c_float, c_float, P]),
    'tdgp_render_fused_workspace_bytes': (c_int64, [c_int, c_int64, c_int, c_int]),
    'tdgp_render_fused': (c_int, [P] * 13 + [c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_int, c_int, c_float, P, c_int64, P]),
    'tdgp_rays_to_image': (c_int, [P, P, c_int, c_int, P]),
    'tdgp_frames_to_grid_u8': (c_int, [P, c_int64, c_int, c_int, c_int, P, c_int, c_int, c_int64, c_int64, c_int, c_int, c_int, c_float, c_float, P]),
    'tdgp_ppl_frames': (c_int, [P, c_int64, c_int, c_int, c_int, c_int, c_int, P, P]),
    'tdgp_pair_sqdist_workspace_bytes': (c_int64, [c_int64, c_int64]),
    'tdgp_pair_sqdist': (c_int, [P, c_int64, c_int64, c_double, P, P, c_int64, P]),
    'tdgp_voxel_coords': (c_int, [P, c_int64, c_int64, c_int, c_float, c_float, c_float, c_float, P]),
    'tdgp_mcubes_workspace_bytes': (c_int64, [c_int, c_int, c_int]),
    'tdgp_mcubes_count': (c_int, [P, c_int, c_int, c_int, c_float, P, c_int64, P]),
    'tdgp_mcubes_emit': (c_int, [P, c_int, c_int, c_int, c_float, P, c_int64, P, c_int64, P, c_int64, P]),
    'tdgp_iso_bracket': (c_int, [P, c_int64, P, c_int64, c_int, c_int, c_float, P, P, P]),
    'tdgp_iso_locate': (c_int, [P, c_int64, P, P, P, c_int64, P, P, P, c_int64, c_int, c_int, c_float, c_float, c_float, P, P, P, P]),
    'tdgp_iso_shade': (c_int, [P, P, P, c_int64, c_int, POINTER(c_float), c_float, POINTER(c_float), POINTER(c_float), P, P, P]),
    'tdgp_mesh_visibility': (c_int, [P, c_int64, P, c_int64, P, P, P, c_int, c_int, c_int, c_float, c_int, P, P]),
    'tdgp_mesh_resolve': (c_int, [P, P, c_int64, P, c_int64, P, P, c_int64, c_float, c_float, P, P, P, P, P, P, P, P]),
    'tdgp_mesh_shade': (c_int, [P, P, P, P, c_int64, c_int, POINTER(c_float), c_float, POINTER(c_float), POINTER(c_float), P, P]),
    'tdgp_mesh_visibility_ms': (c_int, [P, c_int64, P, c_int64, P, P, c_int, c_int, c_int, c_int, c_float, c_int, P, P]),
    'tdgp_mesh_resolve_ms': (c_int, [P, P, c_int64, P, c_int64, P, P, c_int, c_int, c_int, c_int, c_float, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int,
                                     POINTER(c_float), c_float, POINTER(c_float), POINTER(c_float), P, P, P, P, P, P, P]),
    'tdgp_mesh_labels_workspace_bytes': (c_int64, [c_int64, c_int64]),
    'tdgp_mesh_labels': (c_int, [P, c_int64, c_int64, P, P, c_int64, P]),
    'tdgp_mesh_component_ids_workspace_bytes': (c_int64, [c_int64]),
    'tdgp_mesh_component_ids': (c_int, [P, c_int64, P, P, c_int64, P]),
    'tdgp_mesh_component_stats': (c_int, [P, P, c_int64, c_int64, P, c_int64, P, P, P, P, P, P, P, P]),
    'tdgp_mesh_component_sums': (c_int, [P, P, P, c_int64, c_int64, P, P, P, P, P]),
    'tdgp_mesh_compact_workspace_bytes': (c_int64, [c_int64, c_int64]),
    'tdgp_mesh_compact_count': (c_int, [P, c_int64, c_int64, P, P, c_int64, P, c_int64, P]),
    'tdgp_mesh_compact_emit': (c_int, [P, P, c_int64, c_int64, P, P, c_int64, P, c_int64, P, c_int64, P, c_int64, P, POINTER(c_void_p), POINTER(c_void_p),
                                       POINTER(c_int32), c_int, P]),
    'tdgp_mesh_corner_table_workspace_bytes': (c_int64, [c_int64, c_int64]),
    'tdgp_mesh_corner_table': (c_int, [P, c_int64, c_int64, P, P, P, P, c_int64, P]),
    'tdgp_mesh_vertex_normals': (c_int, [P, P, c_int64, c_int64, P, P, c_int, P, P]),
    'tdgp_mesh_boundary_vertices': (c_int, [P, c_int64, c_int64, P, P, P, P]),
    'tdgp_mesh_smooth_step': (c_int, [P, P, c_int64, c_int64, P, P, c_double, P, P, P]),
    'tdgp_mesh_interp_normals': (c_int, [P, P, P, P, P, c_int64, P, c_int64, P, c_int64, P, P, P]),
    'tdgp_mesh_cluster_keys': (c_int, [P, c_int64, POINTER(c_double), POINTER(c_double), P, P]),
    'tdgp_mesh_cluster_ids_workspace_bytes': (c_int64, [c_int64]),
    'tdgp_mesh_cluster_ids': (c_int, [P, P, c_int64, P, P, P, P, c_int64, P]),
    'tdgp_mesh_cluster_triangles_relabel': (c_int, [P, c_int64, c_int64, P, P, P, P]),
    'tdgp_mesh_cluster_triangles_workspace_bytes': (c_int64, [c_int64]),
    'tdgp_mesh_cluster_triangles_count': (c_int, [P, P, c_int64, P, P, c_int64, P]),
    'tdgp_mesh_cluster_triangles_emit': (c_int, [P, c_int64, P, P, c_int64, P, c_int64, P, P]),
    'tdgp_mesh_cluster_place': (c_int, [P, c_int64, P, P, P, c_int64, POINTER(c_double), POINTER(c_double), P, c_int64, P, P, c_int, c_double, P, P]),
    'tdgp_mesh_cluster_attribute': (c_int, [P, c_int, c_int64, P, P, c_int64, P, P]),
    'tdgp_mesh_decimate_quadrics': (c_int, [P, P, c_int64, c_int64, P, P, P, P, P, P]),
    'tdgp_mesh_decimate_candidates': (c_int, [P, P, P, P, P, c_int64, c_int64, P, P, c_double, c_double, P, P, P, P]),
    'tdgp_mesh_decimate_claim': (c_int, [P, P, c_int64, c_int64, P, P, P, P]),
    'tdgp_mesh_decimate_select_workspace_bytes': (c_int64, [c_int64]),
    'tdgp_mesh_decimate_select': (c_int, [P, P, P, P, c_int64, c_int64, P, P, P, c_int64, P]),
    'tdgp_mesh_decimate_apply': (c_int, [P, c_int64, P, c_int64, c_int64, P, P, P, P, P, P, c_int, P, P]),
    'tdgp_mesh_decimate_gather_workspace_bytes': (c_int64, [c_int64]),
    'tdgp_mesh_decimate_gather_count': (c_int, [P, c_int64, P, c_int64, P]),
    'tdgp_mesh_decimate_gather': (c_int, [P, P, c_int, P, c_int64, c_int64, P, c_int64, P, c_int64, P, P, P]),
    'tdgp_mesh_distance_prepare': (c_int, [P, P, c_int64, c_int64, P, P, P, P]),
    'tdgp_mesh_distance_grid_count': (c_int, [P, P, c_int64, POINTER(c_float), c_float, POINTER(c_int), P, P]),
    'tdgp_mesh_distance_scan_workspace_bytes': (c_int64, [c_int64]),
    'tdgp_mesh_distance_grid_emit': (c_int, [P, P, c_int64, POINTER(c_float), c_float, POINTER(c_int), P, c_int64, P, P, c_int64, P]),
    'tdgp_mesh_distance_cell_start': (c_int, [P, c_int64, c_int64, P, P]),
    'tdgp_mesh_distance_closest': (c_int, [P, c_int64, P, P, c_int64, c_int64, P, POINTER(c_float), c_float, POINTER(c_int), P, P, c_int64, c_int, P, P, P, P, P, P]),
    'tdgp_mesh_distance_sample_count': (c_int, [P, P, c_int64, c_int64, P, c_float, P, P]),
    'tdgp_mesh_distance_sample_emit': (c_int, [P, P, c_int64, c_int64, P, c_float, P, c_int64, P, P, P, c_int64, P]),
    'tdgp_mesh_distance_reduce_workspace_bytes': (c_int64, [c_int64]),
    'tdgp_mesh_distance_reduce': (c_int, [P, P, c_int64, P, c_int64, P]),
    'tdgp_mesh_rays_cast': (c_int, [P, P, c_int64, c_double, c_double, P, P, c_int64, c_int64, P, POINTER(c_float), c_float, POINTER(c_int), P, P, c_int64, c_int, c_int,
                                    P, P, P, P, P, P, P, P]),
    'tdgp_mesh_rays_ao': (c_int, [P, P, c_int64, P, c_int, c_int, c_float, c_float, P, P, c_int64, c_int64, POINTER(c_float), c_float, POINTER(c_int), P, P, c_int64, P, P]),
    'tdgp_atlas_points':(c_int, [P, c_int64, P, c_int64, c_int, c_int, c_int, c_int, P, P, P]),
    'tdgp_atlas_texels': (c_int, [P, c_int64, P, c_int64, P, P, P]),
    'tdgp_mesh_sample_texture': (c_int, [P, P, P, P, P, c_int64, P, c_int64, P, c_int64, P, c_int, c_int, c_int, c_int, c_int, P, P]),
    'tdgp_quantile_select_workspace_bytes': (c_int64, [c_int64]),
    'tdgp_quantile_select': (c_int, [P, c_int64, c_int64, c_int64, c_float, P, P, c_int64, P]),
    'tdgp_depth_histc': (c_int, [P, c_int64, c_int64, c_float, c_float, c_int, P, P]),
    'tdgp_pr_pack': (c_int, [P, c_int64, c_int, P, c_int, P, P]),
    'tdgp_pr_kth_workspace_bytes': (c_int64, [c_int64, c_int64, c_int]),
    'tdgp_pr_kth': (c_int, [P, P, c_int64, P, P, c_int64, c_int, c_int, P, P, c_int64, P]),
    'tdgp_pr_member_workspace_bytes': (c_int64, [c_int64, c_int64]),
    'tdgp_pr_member': (c_int, [P, P, c_int64, P, P, P, c_int64, c_int, P, P, c_int64, P]),
    'tdgp_moments_workspace_bytes': (c_int64, [c_int64, c_int]),
    'tdgp_moments_add': (c_int, [P, c_int64, c_int, P, P, P, c_int64, P]),
    'tdgp_gaussian_maha_mode': (c_int, [c_int64, c_int]),
    'tdgp_gaussian_maha_workspace_bytes': (c_int64, [c_int64, c_int]),
    'tdgp_gaussian_maha': (c_int, [P, c_int64, c_int, P, P, P, P, c_int64, P]),
    'tdgp_augment_params': (c_int, [POINTER(c_float), P, c_int, c_int, c_int, c_int, P, P, c_int, c_float, P, P, P, P, P, P]),
    'tdgp_augment_geom': (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P]),
    'tdgp_augment_geom_adj_workspace_bytes': (c_int64, [c_int, c_int, c_int, c_int]),
    'tdgp_augment_geom_adj': (c_int, [P, P, P, P, c_int, c_int, c_int, c_int, P, c_int64, P]),
    'tdgp_augment_color': (c_int, [P, P, P, c_int, c_int, P, P, P, c_int, c_int, c_int, c_int, c_int, P]),
    'tdgp_grads_pack': (c_int, [P, P, c_int, c_int64, c_int, P, c_int64, P]),
    'tdgp_grads_sanitise_norm': (c_int, [P, c_int64, c_int, c_int, P, c_int64, P, P]),
    'tdgp_adam_step': (c_int, [P, P, c_int, c_int64, c_int, P, c_int64, P, c_double, c_double, c_double, c_double, P]),
    'tdgp_ema_update': (c_int, [P, c_int, c_int64, c_int, c_double, P]),
    'tdgp_resample_workspace_bytes': (c_int64, [c_int64, c_int, c_int, c_int, c_int, c_int, c_int]),
    'tdgp_resample_u8': (c_int, [P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P, c_int, P, c_int, c_int, P, c_int64, P]),
    'tdgp_resample_u16': (c_int, [P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P, c_int, P, c_int, c_int, c_int, P, c_int64, P]),
    'tdgp_resample_u8_to_f32_workspace_bytes': (c_int64, [c_int64, c_int, c_int, c_int, c_int, c_int, c_int]),
    'tdgp_resample_u8_to_f32': (c_int, [P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, c_int, P, P, c_int, c_int, c_int, c_int,
                                        c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), P, P, c_int64, P]),
}
EXPORTS = tuple(_PROTOTYPES)

_lib = None
_load_error = None


def load():
    """dlopen the prebuilt library (once).  Raises RuntimeError if it is missing or broken."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if _load_error is not None:
        raise RuntimeError(_load_error)
    if not os.path.exists(LIB_PATH):
        _load_error = (f'{LIB_PATH} not found: the gfx950 HIP library is not built. Run `python -c "import __graft_entry__ as g; '
                       f'g.build()"` (hipcc) first. There is no CPU/PyTorch fallback for the native ops.')
        raise RuntimeError(_load_error)
    try:
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOTYPES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    except (OSError, AttributeError) as e:
        _load_error = f'failed to load {LIB_PATH}: {e}'
        raise RuntimeError(_load_error) from e
    _lib = lib
    return _lib


def available():
    try:
        load()
        return True
    except RuntimeError:
        return False


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else t.data_ptr()


def stream_of(t):
    return torch.cuda.current_stream(t.device).cuda_stream


class Unsupported(RuntimeError):
    """TDGP_EUNSUPPORTED: a valid request this build has no kernel for (include/tdgp.h).  Returned before anything is launched."""


def call(name, *args):
    """Call an entry point; non-zero return -> RuntimeError carrying tdgp_last_error()."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.tdgp_last_error()
        raise (Unsupported if rc == -2 else RuntimeError)(f'{name} failed ({rc}): {msg.decode() if msg else "?"}')


def byte_workspace(query_name, dims, device, refusal, at_least=0):
    """Ask `query_name(*dims)` how many workspace bytes a call needs -> (uint8 tensor of max(need, at_least) bytes on `device`, need).
    A negative answer is the library refusing the sizes: `refusal` (the caller's exception, so every entry point keeps its own type and
    words) is raised before anything is allocated."""
    need = int(getattr(load(), query_name)(*dims))
    if need < 0:
        raise refusal
    return torch.empty([max(need, at_least)], dtype=torch.uint8, device=device), need


def require_cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f'{what} must reside on the GPU (got {getattr(t, "device", type(t))}); the HIP ops have no CPU path')


def f32c(t):
    """Contiguous fp32 view/copy."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def profile_enable(on=True):
    """Start (and clear) / stop per-kernel HIP-event timing inside the library."""
    load().tdgp_profile_enable(int(bool(on)))


def profile_report():
    """-> {kernel: dict(launches, total_ms, avg_ms, min_ms, max_ms)}; blocks until the recorded launches finished."""
    lib = load()
    need = lib.tdgp_profile_report(None, 0)
    buf = ctypes.create_string_buffer(int(need) + 16)
    lib.tdgp_profile_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, n, tot, mn, mx = line.split()
        out[name] = dict(launches=int(n), total_ms=float(tot), avg_ms=float(tot) / max(int(n), 1), min_ms=float(mn), max_ms=float(mx))
    return out


def device_fault(clear=False):
    """The library's device-fault word (include/tdgp.h: a bounded in-kernel wait that ran out); read it after synchronising."""
    return int(load().tdgp_device_fault(int(bool(clear))))


def raise_on_device_fault(where=''):
    """Call AFTER a synchronisation point (an image fetched to the host, the end of a training step, a graph replay whose outputs were read):
    a launch whose bounded in-kernel wait ran out has set the fault word -- its results are invalid.  Reads, clears and raises; the C side
    only notices at the entry of the NEXT field / per-ray call, which the last forward of a run never reaches."""
    code = device_fault(clear=True)
    if code:
        raise RuntimeError(f'libtdgp_hip: device fault {code} reported{" in " + where if where else ""}: a bounded in-kernel wait ran out, '
                           'the results of that launch are invalid (the fault word has been cleared)')


def set_conv_arith(mode):
    """0 (default): fp32 MFMA, Winograd F(4x4,3x3) / F(2x2,3x3) on the layers where they pay; 2: direct sums only; 3: as 0 without F(4x4); 1: split-bf16 (3 x bf16 pieces per operand, 6 piece products, fp32 accumulation) for the 3x3 stride-1
    convolutions with W % 32 == 0 and >= 256 output tiles.  Process-wide; returns the previous mode."""
    lib = load()
    prev = int(lib.tdgp_set_conv_arith(int(mode)))
    if prev < 0:
        msg = lib.tdgp_last_error()
        raise RuntimeError(f'tdgp_set_conv_arith failed ({prev}): {msg.decode() if msg else "?"}')
    return prev
