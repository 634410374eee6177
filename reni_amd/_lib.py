"""ctypes binding of libreni_hip.so (C ABI in include/reni_hip.h).

The product path has NO CPU fallback: if the HIP library is missing the import of any compute
entry point raises, loudly.  (The CPU oracle under oracle/ is test infrastructure and is never
imported from here.)
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_float, c_int32, c_int64, c_size_t, c_uint32, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RENI_HIP_LIB") or os.path.join(_HERE, "lib", "libreni_hip.so")  # env override: kernel experiments

RENI_OK = 0
EQ = {"None": 0, None: 0, "SO2": 1, "SO3": 2}
ACT = {None: 0, "None": 0, "none": 0, "tanh": 1, "exp": 2}
DTYPE = {"f32": 0, "fp32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}
LOSS_MSE, LOSS_TEST = 0, 1
LOSS_KIND = {"mse": LOSS_MSE, "test": LOSS_TEST}
NEED_DW, NEED_DZ, WEIGHT_SPARSE, WEIGHT_COMPACT, WEIGHT_COS_CONSTANT = 1, 2, 4, 8, 16
COND_CONCAT, COND_FILM = 0, 1
ROTATE_MODE = {"nearest": 0, "bilinear": 1}
LOBE_KIND = {"phong": 0, "blinn": 1, "ggx": 2}  # RENI_LOBE_*
SPACE = {"stored": 0, "linear": 1, "srgb": 2}
SSIM_MODE = {"sphere": 0, "planar": 1}
VIS_NO_CULL = 1  # RENI_VIS_NO_CULL
SHADE_TERMS_DS = 1  # RENI_SHADE_TERMS_DS
TEX_WRAP = {"clamp": 0, "repeat": 1}  # RENI_TEX_*
LAPLACIAN = {"uniform": 0, "cot": 1}  # RENI_LAPLACIAN_*

# every symbol include/reni_hip.h declares (tests check the library exports all of them)
EXPORTS = (
    "reni_last_error", "reni_plan_create", "reni_plan_destroy", "reni_param_count", "reni_in_features",
    "reni_workspace_bytes", "reni_forward", "reni_forward_loss_backward", "reni_backward",
    "reni_forward_loss_backward_rows", "reni_train_step_rows", "reni_train_step_rows_dp", "reni_latent_step_rows", "reni_latent_step_rows_cached", "reni_weight_lists_bytes", "reni_weight_lists_build", "reni_adam_step", "reni_adam_rows_step", "reni_adam_step2", "reni_selftest_layouts", "reni_launch_info", "reni_path_info", "reni_launch_count", "reni_set_grad_ready_event", "reni_profile_enable", "reni_profile_read", "reni_profile_read_kind", "reni_profile_minmax", "reni_probe_tr",
    "reni_film_forward", "reni_film_forward_loss_backward", "reni_film_backward",
    "reni_film_map_param_count", "reni_film_model_forward", "reni_film_model_forward_loss_backward",
    "reni_film_model_backward",
    "reni_envmap_shade_workspace_bytes", "reni_envmap_shade", "reni_envmap_shade_backward",
    "reni_raster_workspace_bytes", "reni_mesh_vertex_normals", "reni_rasterize_mesh",
    "reni_mesh_vertex_normals_backward", "reni_gbuffer_backward_workspace_bytes", "reni_gbuffer_backward",
    "reni_soft_silhouette_workspace_bytes", "reni_soft_silhouette", "reni_soft_silhouette_backward_workspace_bytes",
    "reni_soft_silhouette_backward",
    "reni_gbuffer_backward_camera_workspace_bytes", "reni_gbuffer_backward_camera",
    "reni_soft_silhouette_backward_camera_workspace_bytes", "reni_soft_silhouette_backward_camera",
    "reni_mesh_regularizers_workspace_bytes", "reni_mesh_regularizers",
    "reni_nearest_points_workspace_bytes", "reni_nearest_points", "reni_chamfer_grad",
    "reni_mesh_sample_table_workspace_bytes", "reni_mesh_sample_table", "reni_mesh_sample_points",
    "reni_nearest_faces_workspace_bytes", "reni_nearest_faces", "reni_faces_nearest_points_workspace_bytes", "reni_faces_nearest_points",
    "reni_knn_points_workspace_bytes", "reni_knn_points", "reni_cloud_normals",
    "reni_mesh_visibility_accel_bytes", "reni_mesh_visibility_prepare", "reni_mesh_visibility",
    "reni_envmap_shade_masked", "reni_envmap_shade_masked_backward",
    "reni_envmap_shade_terms_workspace_bytes", "reni_envmap_shade_terms", "reni_envmap_shade_terms_backward",
    "reni_envmap_shade_terms_dnormals_workspace_bytes", "reni_envmap_shade_terms_dnormals",
    "reni_envmap_shade_ggx_workspace_bytes", "reni_envmap_shade_ggx", "reni_envmap_shade_ggx_backward",
    "reni_envmap_shade_ggx_dpixel_workspace_bytes", "reni_envmap_shade_ggx_dpixel",
    "reni_sg_workspace_bytes", "reni_sg_render", "reni_sg_loss_grad", "reni_sh_project", "reni_sh_reconstruct",
    "reni_diffuse_workspace_bytes", "reni_diffuse_convolve", "reni_sh_irradiance_l2",
    "reni_lobe_workspace_bytes", "reni_lobe_convolve", "reni_envmap_lookup",
    "reni_lobe_denominators_workspace_bytes", "reni_lobe_denominators", "reni_lobe_backward_workspace_bytes",
    "reni_lobe_convolve_backward", "reni_envmap_lookup_taps", "reni_envmap_lookup_backward",
    "reni_envmap_lookup_dquery", "reni_ggx_dfg",
    "reni_mesh_pixel_uv", "reni_texture_taps", "reni_texture_pyramid", "reni_texture_pyramid_backward", "reni_texture_fetch",
    "reni_texture_fetch_backward",
    "reni_image_workspace_bytes", "reni_unnormalise_srgb", "reni_minmax_normalise",
    "reni_minmax_batch_workspace_bytes", "reni_minmax_normalise_batch",
    "reni_resample", "reni_blur_workspace_bytes", "reni_gaussian_blur", "reni_rotate_envmap",
    "reni_pair_stats_workspace_bytes", "reni_pair_stats", "reni_ssim",
    "reni_light_table_workspace_bytes", "reni_light_table_build", "reni_light_sample", "reni_lights_irradiance",
    "reni_rccl_unique_id", "reni_rccl_comm_create", "reni_rccl_comm_destroy", "reni_allreduce_grads",
)


class reni_desc(Structure):
    _fields_ = [
        ("equivariance", c_int32), ("ndims", c_int32), ("hidden_features", c_int32),
        ("hidden_layers", c_int32), ("out_features", c_int32), ("last_layer_linear", c_int32),
        ("output_activation", c_int32), ("first_omega_0", c_float), ("hidden_omega_0", c_float),
        ("dtype", c_int32), ("conditioning", c_int32), ("mapping_layers", c_int32), ("mapping_features", c_int32),
    ]


class RENILibraryError(RuntimeError):
    pass


_lib = None


def load():
    """Load libreni_hip.so (built by reni_amd/csrc/build.sh or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RENILibraryError(
            f"{LIB_PATH} is missing: the RENI HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or reni_amd/csrc/build.sh). "
            "There is no CPU fallback."
        )
    lib = ctypes.CDLL(LIB_PATH)
    i64x3 = POINTER(c_int64)
    lib.reni_last_error.argtypes = []
    lib.reni_last_error.restype = c_char_p
    lib.reni_plan_create.argtypes = [POINTER(reni_desc), POINTER(c_void_p)]
    lib.reni_plan_create.restype = c_int32
    lib.reni_plan_destroy.argtypes = [c_void_p]
    lib.reni_plan_destroy.restype = None
    lib.reni_param_count.argtypes = [c_void_p]
    lib.reni_param_count.restype = c_int64
    lib.reni_in_features.argtypes = [c_void_p]
    lib.reni_in_features.restype = c_int32
    lib.reni_workspace_bytes.argtypes = [c_void_p, c_int64, c_int64, c_uint32]
    lib.reni_workspace_bytes.restype = c_size_t
    lib.reni_forward.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                 c_void_p, c_size_t, c_void_p]
    lib.reni_forward.restype = c_int32
    # the twins' shared runs of parameters, in the header's order (tests/test_api_cpu.py holds every list against its prototype)
    rows = [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p]  # plan, B, P, Z_table, n_rows, idx
    loss = [c_void_p, c_int64, c_void_p, c_void_p, i64x3, c_void_p, i64x3, c_int32, c_float, c_float]  # D, dbs, params, target .. beta
    grads = [c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]  # flags, out, loss_terms, dZ, dparams, ws ..
    lib.reni_forward_loss_backward.argtypes = rows[:4] + loss + grads
    lib.reni_forward_loss_backward_rows.argtypes = rows + loss + grads
    adam = [c_float, c_float, c_float, c_float, c_int64]  # lr, b1, b2, eps, step
    step_head = rows + [c_void_p] + loss + [c_void_p, c_void_p, c_void_p, c_void_p] + adam + [c_float]  # idx_next; m / v x 2; grad_scale
    step_tail = [POINTER(c_uint32), c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]  # stage_state, loss_terms, dZ, dparams, ws ..
    lib.reni_train_step_rows.argtypes = step_head + step_tail
    lib.reni_train_step_rows_dp.argtypes = step_head + [c_void_p, c_int32] + step_tail  # comm, overlap
    latent_tail = [c_void_p, c_void_p] + adam + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]  # m, v; loss_terms, dZ, ws ..
    lib.reni_latent_step_rows.argtypes = rows + loss + [c_uint32] + latent_tail
    lib.reni_latent_step_rows_cached.argtypes = rows + loss + [c_uint32, c_void_p] + latent_tail  # flags, weight_lists
    for fn in (lib.reni_forward_loss_backward, lib.reni_forward_loss_backward_rows, lib.reni_train_step_rows,
               lib.reni_train_step_rows_dp, lib.reni_latent_step_rows, lib.reni_latent_step_rows_cached):
        fn.restype = c_int32
    lib.reni_weight_lists_bytes.argtypes = [c_int64, c_int64]
    lib.reni_weight_lists_bytes.restype = c_size_t
    lib.reni_weight_lists_build.argtypes = [c_int64, c_int64, c_void_p, i64x3, c_uint32, c_void_p, c_size_t, POINTER(c_int32), c_void_p]
    lib.reni_weight_lists_build.restype = c_int32
    lib.reni_adam_step2.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                    c_int64, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_int64, c_float,
                                    c_void_p]
    lib.reni_adam_step2.restype = c_int32
    lib.reni_backward.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                  c_uint32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_backward.restype = c_int32
    lib.reni_film_forward.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_film_forward.restype = c_int32
    lib.reni_film_forward_loss_backward.argtypes = [
        c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, i64x3, c_void_p, i64x3,
        c_int32, c_float, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_film_forward_loss_backward.restype = c_int32
    lib.reni_film_backward.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_film_backward.restype = c_int32
    lib.reni_film_map_param_count.argtypes = [c_void_p]
    lib.reni_film_map_param_count.restype = c_int64
    lib.reni_film_model_forward.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_film_model_forward.restype = c_int32
    lib.reni_film_model_forward_loss_backward.argtypes = [
        c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, i64x3, c_void_p, i64x3,
        c_int32, c_float, c_float, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_film_model_forward_loss_backward.restype = c_int32
    lib.reni_film_model_backward.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                             c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_film_model_backward.restype = c_int32
    lib.reni_adam_step.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float,
                                   c_float, c_int64, c_float, c_void_p]
    lib.reni_adam_step.restype = c_int32
    lib.reni_adam_rows_step.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_float,
                                        c_float, c_float, c_float, c_int64, c_float, c_void_p]
    lib.reni_adam_rows_step.restype = c_int32
    lib.reni_selftest_layouts.argtypes = [POINTER(c_int32), c_int32]
    lib.reni_selftest_layouts.restype = c_int32
    lib.reni_launch_info.argtypes = [c_void_p, c_int64, c_int64, POINTER(c_int32)]
    lib.reni_launch_info.restype = c_int32
    lib.reni_path_info.argtypes = [c_void_p, c_int64, c_int64, c_uint32, POINTER(c_int32)]
    lib.reni_path_info.restype = c_int32
    lib.reni_set_grad_ready_event.argtypes = [c_void_p]
    lib.reni_set_grad_ready_event.restype = c_int32
    lib.reni_launch_count.argtypes = [c_int32]
    lib.reni_launch_count.restype = c_int64
    lib.reni_profile_enable.argtypes = [c_int32]
    lib.reni_profile_enable.restype = c_int32
    lib.reni_profile_read.argtypes = [POINTER(ctypes.c_double), POINTER(c_int64), c_int32]
    lib.reni_profile_read.restype = c_int32
    lib.reni_profile_read_kind.argtypes = [c_int32, POINTER(ctypes.c_double), POINTER(c_int64), c_int32]
    lib.reni_profile_read_kind.restype = c_int32
    lib.reni_profile_minmax.argtypes = [c_int32, POINTER(ctypes.c_double), POINTER(ctypes.c_double)]
    lib.reni_profile_minmax.restype = c_int32
    lib.reni_probe_tr.argtypes = [c_void_p, c_int32, c_void_p]
    lib.reni_probe_tr.restype = c_int32
    lib.reni_envmap_shade_workspace_bytes.argtypes = [c_int64, c_int64, c_int64]
    lib.reni_envmap_shade_workspace_bytes.restype = c_size_t
    for fn in (lib.reni_envmap_shade, lib.reni_envmap_shade_backward):
        fn.argtypes = [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_float, c_float, c_float, c_void_p, c_int64,
                       c_void_p, c_float, c_float, c_float, c_void_p, c_void_p, c_size_t, c_void_p]
        fn.restype = c_int32
    lib.reni_raster_workspace_bytes.argtypes = [c_int64, c_int64, c_int64, c_int64]
    lib.reni_raster_workspace_bytes.restype = c_size_t
    lib.reni_mesh_vertex_normals.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.reni_mesh_vertex_normals.restype = c_int32
    lib.reni_rasterize_mesh.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_float), POINTER(c_float), c_float,
                                        c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_size_t, c_void_p]
    lib.reni_rasterize_mesh.restype = c_int32
    lib.reni_mesh_vertex_normals_backward.argtypes = [c_int64, c_int64] + [c_void_p] * 7
    lib.reni_mesh_vertex_normals_backward.restype = c_int32
    lib.reni_gbuffer_backward_workspace_bytes.argtypes = [c_int64, c_int64, c_int64, c_int64]
    lib.reni_gbuffer_backward_workspace_bytes.restype = c_size_t
    gbuf = [c_int64, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_float), POINTER(c_float), c_float, c_int64, c_int64]
    lib.reni_gbuffer_backward.argtypes = gbuf + [c_void_p] * 9 + [c_size_t, c_void_p]  # p2f, table, lists, gN, gX, grad_verts, ws ..
    lib.reni_gbuffer_backward.restype = c_int32
    for fn in (lib.reni_soft_silhouette_workspace_bytes, lib.reni_soft_silhouette_backward_workspace_bytes):
        fn.argtypes = [c_int64, c_int64, c_int64, c_int64]
        fn.restype = c_size_t
    sil = [c_int64, c_int64, c_void_p, c_void_p, POINTER(c_float), POINTER(c_float), c_float, c_int64, c_int64, c_float, c_float]
    lib.reni_soft_silhouette.argtypes = sil + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]  # alpha, trans, ws ..
    lib.reni_soft_silhouette.restype = c_int32
    lib.reni_soft_silhouette_backward.argtypes = sil + [c_void_p] * 6 + [c_size_t, c_void_p]  # trans, gA, lists, grad_verts, ws ..
    lib.reni_soft_silhouette_backward.restype = c_int32
    # the camera variants: the same arguments with grad_camera [13] behind grad_verts
    for fn in (lib.reni_gbuffer_backward_camera_workspace_bytes, lib.reni_soft_silhouette_backward_camera_workspace_bytes):
        fn.argtypes = [c_int64, c_int64, c_int64, c_int64]
        fn.restype = c_size_t
    lib.reni_gbuffer_backward_camera.argtypes = gbuf + [c_void_p] * 10 + [c_size_t, c_void_p]
    lib.reni_gbuffer_backward_camera.restype = c_int32
    lib.reni_soft_silhouette_backward_camera.argtypes = sil + [c_void_p] * 7 + [c_size_t, c_void_p]
    lib.reni_soft_silhouette_backward_camera.restype = c_int32
    lib.reni_mesh_regularizers_workspace_bytes.argtypes = [c_int64, c_int64, c_int64]
    lib.reni_mesh_regularizers_workspace_bytes.restype = c_size_t
    # V, F, E, H, NC; verts, faces and the eight lists; three weights, target_length; method; values, grad_verts, ws ..
    lib.reni_mesh_regularizers.argtypes = ([c_int64] * 5 + [c_void_p] * 10 + [c_float] * 4 + [c_int32, c_void_p, c_void_p, c_void_p,
                                                                                              c_size_t, c_void_p])
    lib.reni_mesh_regularizers.restype = c_int32
    lib.reni_nearest_points_workspace_bytes.argtypes = [c_int64, c_int64]
    lib.reni_nearest_points_workspace_bytes.restype = c_size_t
    # N, M; x, y; slices; dist2, idx, ws ..
    lib.reni_nearest_points.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_nearest_points.restype = c_int32
    # N, M; x, y, idx_xy, order, offsets; w_x, w_y; g, grad_x
    lib.reni_chamfer_grad.argtypes = [c_int64, c_int64] + [c_void_p] * 5 + [c_float, c_float, c_void_p, c_void_p, c_void_p]
    lib.reni_chamfer_grad.restype = c_int32
    lib.reni_mesh_sample_table_workspace_bytes.argtypes = [c_int64]
    lib.reni_mesh_sample_table_workspace_bytes.restype = c_size_t
    lib.reni_mesh_sample_table.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_mesh_sample_table.restype = c_int32
    # V, F, S; faces, table, u; tap_index, tap_weight, face_idx
    lib.reni_mesh_sample_points.argtypes = [c_int64] * 3 + [c_void_p] * 7
    lib.reni_mesh_sample_points.restype = c_int32
    for name in ("reni_nearest_faces", "reni_faces_nearest_points"):
        getattr(lib, name + "_workspace_bytes").argtypes = [c_int64] * 3
        getattr(lib, name + "_workspace_bytes").restype = c_size_t
        # N, V, F; points, verts, faces; slices; dist2, idx, tap_index, tap_weight, ws ..
        getattr(lib, name).argtypes = [c_int64] * 3 + [c_void_p] * 3 + [c_int32] + [c_void_p] * 5 + [c_size_t, c_void_p]
        getattr(lib, name).restype = c_int32
    lib.reni_knn_points_workspace_bytes.argtypes = [c_int64] * 3
    lib.reni_knn_points_workspace_bytes.restype = c_size_t
    # N, M, K; x, y; slices; dist2, idx, ws ..
    lib.reni_knn_points.argtypes = [c_int64] * 3 + [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_knn_points.restype = c_int32
    # N, M, K; y, idx, viewpoint; normals, eigenvalues
    lib.reni_cloud_normals.argtypes = [c_int64] * 3 + [c_void_p] * 6
    lib.reni_cloud_normals.restype = c_int32
    lib.reni_mesh_visibility_accel_bytes.argtypes = [c_int64]
    lib.reni_mesh_visibility_accel_bytes.restype = c_size_t
    lib.reni_mesh_visibility_prepare.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_mesh_visibility_prepare.restype = c_int32
    lib.reni_mesh_visibility.argtypes = [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_float,
                                         c_uint32, c_void_p, c_void_p]
    lib.reni_mesh_visibility.restype = c_int32
    for fn in (lib.reni_envmap_shade_masked, lib.reni_envmap_shade_masked_backward):  # the shader's list + vis, vis_batch_stride
        fn.argtypes = [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_float, c_float, c_float, c_void_p, c_int64,
                       c_void_p, c_float, c_float, c_float, c_void_p, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]
        fn.restype = c_int32
    lib.reni_envmap_shade_terms_workspace_bytes.argtypes = [c_int64, c_int64, c_int64, c_uint32]
    lib.reni_envmap_shade_terms_workspace_bytes.restype = c_size_t
    terms = [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_float, c_float, c_float, c_void_p, c_int64]  # B, NP, J .. dirs_batch_stride
    mats = [c_void_p, c_int64, c_void_p, c_int64]  # shininess + stride, vis + stride
    lib.reni_envmap_shade_terms.argtypes = terms + [c_void_p] + mats + [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_envmap_shade_terms.restype = c_int32
    lib.reni_envmap_shade_terms_backward.argtypes = terms + mats + [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_envmap_shade_terms_backward.restype = c_int32
    lib.reni_envmap_shade_terms_dnormals_workspace_bytes.argtypes = [c_int64, c_int64, c_int64]
    lib.reni_envmap_shade_terms_dnormals_workspace_bytes.restype = c_size_t
    lib.reni_envmap_shade_terms_dnormals.argtypes = (terms + [c_void_p] + mats +  # .. light_colors, materials, gD, gS, d_normals, ws ..
                                                     [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p])
    lib.reni_envmap_shade_terms_dnormals.restype = c_int32
    for fn in (lib.reni_envmap_shade_ggx_workspace_bytes, lib.reni_envmap_shade_ggx_dpixel_workspace_bytes):
        fn.argtypes = [c_int64, c_int64, c_int64]
        fn.restype = c_size_t
    # the terms' lists with alpha + stride in the shininess's place
    lib.reni_envmap_shade_ggx.argtypes = terms + [c_void_p] + mats + [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_envmap_shade_ggx.restype = c_int32
    lib.reni_envmap_shade_ggx_backward.argtypes = terms + mats + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_envmap_shade_ggx_backward.restype = c_int32
    lib.reni_envmap_shade_ggx_dpixel.argtypes = (terms + [c_void_p] + mats +  # .. light_colors, alpha, vis, gD, gS0, gS1, d_alpha, d_normals, ws ..
                                                 [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p])
    lib.reni_envmap_shade_ggx_dpixel.restype = c_int32
    lib.reni_sg_workspace_bytes.argtypes = [c_int64, c_int64, c_int64, c_int64]
    lib.reni_sg_workspace_bytes.restype = c_size_t
    lib.reni_sg_render.argtypes = [c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p,
                                   c_void_p]
    lib.reni_sg_render.restype = c_int32
    lib.reni_sg_loss_grad.argtypes = [c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p,
                                      c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_size_t, c_void_p]
    lib.reni_sg_loss_grad.restype = c_int32
    for fn in (lib.reni_sh_project, lib.reni_sh_reconstruct):
        fn.argtypes = [c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        fn.restype = c_int32
    lib.reni_diffuse_workspace_bytes.argtypes = [c_int64, c_int64, c_int64]
    lib.reni_diffuse_workspace_bytes.restype = c_size_t
    lib.reni_diffuse_convolve.argtypes = [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                          c_int64, c_float, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_diffuse_convolve.restype = c_int32
    lib.reni_sh_irradiance_l2.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]
    lib.reni_sh_irradiance_l2.restype = c_int32
    lib.reni_lobe_workspace_bytes.argtypes = [c_int64, c_int64, c_int64, c_int64]
    lib.reni_lobe_workspace_bytes.restype = c_size_t
    lib.reni_lobe_convolve.argtypes = [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                       c_int64, c_int32, POINTER(c_int32), POINTER(c_float), c_int32, c_float, c_void_p,
                                       c_void_p, c_size_t, c_void_p]
    lib.reni_lobe_convolve.restype = c_int32
    lib.reni_envmap_lookup.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, POINTER(c_int64), c_void_p,
                                       c_int64, c_void_p, c_int64, c_float, c_void_p, c_void_p]
    lib.reni_envmap_lookup.restype = c_int32
    lib.reni_lobe_denominators_workspace_bytes.argtypes = [c_int64, c_int64, c_int64]
    lib.reni_lobe_denominators_workspace_bytes.restype = c_size_t
    lib.reni_lobe_denominators.argtypes = [c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int32, POINTER(c_int32),
                                           POINTER(c_float), c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_lobe_denominators.restype = c_int32
    lib.reni_lobe_backward_workspace_bytes.argtypes = [c_int64, c_int64, c_int64, c_int64]
    lib.reni_lobe_backward_workspace_bytes.restype = c_size_t
    lib.reni_lobe_convolve_backward.argtypes = [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                                POINTER(c_int32), POINTER(c_float), c_int32, c_float, c_void_p, c_void_p,
                                                c_int64, c_int64, c_int64, c_void_p, c_size_t, c_void_p]
    lib.reni_lobe_convolve_backward.restype = c_int32
    lib.reni_envmap_lookup_taps.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                            c_float, c_void_p, c_void_p, c_void_p]
    lib.reni_envmap_lookup_taps.restype = c_int32
    lib.reni_envmap_lookup_backward.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_void_p]
    lib.reni_envmap_lookup_backward.restype = c_int32
    lib.reni_envmap_lookup_dquery.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, POINTER(c_int64), c_void_p,
                                              c_int64, c_void_p, c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.reni_envmap_lookup_dquery.restype = c_int32
    lib.reni_ggx_dfg.argtypes = [c_int64, c_int64, c_float, c_int64, c_int64, c_void_p, c_void_p]
    lib.reni_ggx_dfg.restype = c_int32
    lib.reni_mesh_pixel_uv.argtypes = [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_float),
                                       POINTER(c_float), c_float, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.reni_mesh_pixel_uv.restype = c_int32
    lib.reni_texture_taps.argtypes = [c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_float, c_int32, c_int32,
                                      c_void_p, c_void_p, c_void_p]
    lib.reni_texture_taps.restype = c_int32
    for fn in (lib.reni_texture_pyramid, lib.reni_texture_pyramid_backward):
        fn.argtypes = [c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p]
        fn.restype = c_int32
    lib.reni_texture_fetch.argtypes = [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.reni_texture_fetch.restype = c_int32
    lib.reni_texture_fetch_backward.argtypes = [c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                                c_void_p]
    lib.reni_texture_fetch_backward.restype = c_int32
    lib.reni_image_workspace_bytes.argtypes = [c_int64, c_int64, c_int64]
    lib.reni_image_workspace_bytes.restype = c_size_t
    lib.reni_unnormalise_srgb.argtypes = [c_int64, c_int64, c_int64, c_void_p, POINTER(c_int64), c_int32, ctypes.c_double,
                                          ctypes.c_double, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_unnormalise_srgb.restype = c_int32
    lib.reni_minmax_normalise.argtypes = [c_int64, c_void_p, ctypes.c_double, ctypes.c_double, c_void_p, c_void_p, c_size_t,
                                          c_void_p]
    lib.reni_minmax_normalise.restype = c_int32
    lib.reni_minmax_batch_workspace_bytes.argtypes = [c_int64]
    lib.reni_minmax_batch_workspace_bytes.restype = c_size_t
    lib.reni_minmax_normalise_batch.argtypes = [c_int64, c_int64, c_void_p, ctypes.c_double, ctypes.c_double, c_int32, c_void_p,
                                                c_void_p, c_size_t, c_void_p]
    lib.reni_minmax_normalise_batch.restype = c_int32
    lib.reni_resample.argtypes = [c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, POINTER(c_int64), c_void_p,
                                  c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]
    lib.reni_resample.restype = c_int32
    lib.reni_blur_workspace_bytes.argtypes = [c_int64, c_int64, c_int64]
    lib.reni_blur_workspace_bytes.restype = c_size_t
    lib.reni_gaussian_blur.argtypes = [c_int64, c_int64, c_int64, c_void_p, POINTER(c_int64), c_void_p, c_int32, c_void_p,
                                       c_void_p, c_size_t, c_void_p]
    lib.reni_gaussian_blur.restype = c_int32
    lib.reni_rotate_envmap.argtypes = [c_int64, c_int64, c_int64, c_int64, c_void_p, POINTER(c_int64), c_void_p, c_int64, c_void_p,
                                       c_int64, c_void_p, c_void_p, c_int32, c_void_p, c_void_p]
    lib.reni_rotate_envmap.restype = c_int32
    lib.reni_pair_stats_workspace_bytes.argtypes = [c_int64, c_int64, c_int64]
    lib.reni_pair_stats_workspace_bytes.restype = c_size_t
    pair = [c_int64, c_int64, c_int64, c_void_p, POINTER(c_int64), c_void_p, POINTER(c_int64), c_void_p, POINTER(c_int64), c_int32,
            ctypes.c_double, ctypes.c_double, c_void_p]  # B, H, W, pred + strides, target + strides, weight + strides, space, minmax, exposure
    lib.reni_pair_stats.argtypes = pair + [c_void_p, c_void_p, c_size_t, c_void_p]
    lib.reni_pair_stats.restype = c_int32
    lib.reni_ssim.argtypes = pair + [c_float, c_int32, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]  # L, mode, out, map_out, ws ..
    lib.reni_ssim.restype = c_int32
    lib.reni_light_table_workspace_bytes.argtypes = [c_int64, c_int64, c_int64]
    lib.reni_light_table_workspace_bytes.restype = c_size_t
    image = [c_void_p, POINTER(c_int64)]  # img + strides
    space = [c_int32, ctypes.c_double, ctypes.c_double]  # space, minmax
    lib.reni_light_table_build.argtypes = ([c_int64, c_int64, c_int64] + image + [c_void_p, POINTER(c_int64)] + space +  # B, H, W .. mask + strides ..
                                           [c_void_p, ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p])  # solid_angle, uniform_mix, pmf, cond, marg, ws ..
    lib.reni_light_table_build.restype = c_int32
    lib.reni_light_sample.argtypes = ([c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p] + image + space +  # B, H, W, S, pmf, cond, marg ..
                                      [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32] +  # u + stride, dirs_table, solid_angle, row_cos, texel_weight, jitter
                                      [c_void_p] * 5 + [c_void_p])  # index, dirs, pdf, radiance, colors; stream
    lib.reni_light_sample.restype = c_int32
    lib.reni_lights_irradiance.argtypes = [c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_float, c_void_p, c_void_p]
    lib.reni_lights_irradiance.restype = c_int32
    lib.reni_rccl_unique_id.argtypes = [c_void_p]
    lib.reni_rccl_unique_id.restype = c_int32
    lib.reni_rccl_comm_create.argtypes = [c_void_p, c_int32, c_int32, POINTER(c_void_p)]
    lib.reni_rccl_comm_create.restype = c_int32
    lib.reni_rccl_comm_destroy.argtypes = [c_void_p]
    lib.reni_rccl_comm_destroy.restype = c_int32
    lib.reni_allreduce_grads.argtypes = [c_void_p, c_void_p, c_size_t, c_float, c_void_p]
    lib.reni_allreduce_grads.restype = c_int32
    _lib = lib
    return lib


def check(rc: int):
    if rc != RENI_OK:
        msg = load().reni_last_error().decode("utf-8", "replace")
        raise RENILibraryError(f"libreni_hip error {rc}: {msg}")
