"""Python binding of the C++ Trident::Renderer shim (libtrident_renderer.so, host/include/trident_app.h).

The shim is the reference's renderer API (Renderer/RenderCommand over an ECS registry and the
editor/runtime cameras) restated in C++ on top of the HIP C-ABI. This binding drives it the way
Trident-Forge's ApplicationLayer does, for tests. No CPU fallback: the library must be built.
"""
import ctypes as C
import os

import numpy as np

from . import abi
from .raster import PKG_ROOT, TriError

LIB_PATH = os.path.join(PKG_ROOT, "lib", "libtrident_renderer.so")

PRIMITIVE = {"none": 0, "cube": 1, "sphere": 2, "quad": 3}
LIGHT = {"directional": 0, "point": 1}

_f3 = C.POINTER(C.c_float)
_APP_FUNCTIONS = [
    ("trident_app_create", C.c_int, [C.c_uint32, C.POINTER(C.c_void_p)]),
    ("trident_app_destroy", None, [C.c_void_p]),
    ("trident_app_append_mesh", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, _f3, C.c_float,
                                          C.c_float, C.c_char_p, C.POINTER(C.c_uint32)]),
    ("trident_app_upload_texture", C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("trident_app_add_mesh_entity", C.c_int, [C.c_void_p, C.c_int, C.c_uint32, _f3, _f3, _f3, C.POINTER(C.c_uint32)]),
    ("trident_app_set_entity_texture", C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p]),
    ("trident_app_set_entity_transform", C.c_int, [C.c_void_p, C.c_uint32, _f3, _f3, _f3]),
    ("trident_app_set_entity_visible", C.c_int, [C.c_void_p, C.c_uint32, C.c_int]),
    ("trident_app_set_entity_bones", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    ("trident_app_set_entities_bones", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    ("trident_app_set_assets_dir", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint32]),
    ("trident_app_viewport_texture", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(abi.TriImage)]),
    ("trident_app_set_light_shadow_caster", C.c_int, [C.c_void_p, C.c_uint32, C.c_int]),
    ("trident_app_set_shadow_map_size", C.c_int, [C.c_void_p, C.c_uint32]),
    ("trident_app_set_device_count", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    ("trident_app_add_sprite_entity", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_float, C.POINTER(C.c_uint32)]),
    ("trident_app_set_sprite_visible", C.c_int, [C.c_void_p, C.c_uint32, C.c_int]),
    ("trident_app_entity_sprite", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float * 10)]),
    ("trident_app_shadow_config", C.c_int, [C.c_void_p, C.POINTER(abi.TriShadowConfig), C.POINTER(C.c_int)]),
    ("trident_app_geometry_uploads", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("trident_load_image", C.c_int, [C.c_char_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32)]),
    ("trident_load_default_skybox", C.c_int, [C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.c_char_p,
                                              C.c_uint32]),
    ("trident_load_default_skybox_ex", C.c_int, [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint32]),
    ("trident_load_skybox", C.c_int, [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("trident_float_to_half", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("trident_app_add_light", C.c_int, [C.c_void_p, C.c_int, _f3, _f3, _f3, C.c_float, C.c_float, C.c_int,
                                        C.POINTER(C.c_uint32)]),
    ("trident_app_set_camera", C.c_int, [C.c_void_p, C.c_int, _f3, _f3, C.c_float, C.c_float, C.c_float, C.c_int]),
    ("trident_app_set_viewport", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("trident_app_set_clear_color", C.c_int, [C.c_void_p, _f3]),
    ("trident_app_set_skybox", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("trident_app_draw_frame", C.c_int, [C.c_void_p]),
    ("trident_app_finish_frame", C.c_int, [C.c_void_p]),
    ("trident_app_set_frames_in_flight", C.c_int, [C.c_void_p, C.c_uint32]),
    ("trident_app_read_pixels", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("trident_app_frame_inputs", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(abi.TriGlobalUbo), C.c_void_p, C.c_uint32,
                                           C.POINTER(C.c_uint32)]),
    ("trident_app_geometry", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_size_t), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_app_materials", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_app_frame_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("trident_app_import_model", C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_app_save_scene", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p]),
    ("trident_app_load_scene", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32)]),
    ("trident_app_use_scene_camera", C.c_int, [C.c_void_p]),
    ("trident_app_entity_transform", C.c_int, [C.c_void_p, C.c_uint32, _f3]),
    ("trident_app_entity_mesh", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]),
    ("trident_app_entity_count", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    ("trident_app_set_present_extent", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    ("trident_app_set_ai_blend_strength", C.c_int, [C.c_void_p, C.c_float]),
    ("trident_app_submit_ai_frame", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("trident_app_read_present", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("trident_app_set_recording", C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p,
                                            C.POINTER(C.c_uint32 * 2)]),
    ("trident_app_recording_state", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    ("trident_app_set_recording_quality", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    ("trident_video_create", C.c_int, [C.POINTER(C.c_void_p)]),
    ("trident_video_destroy", None, [C.c_void_p]),
    ("trident_video_begin", C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("trident_video_submit_rgba", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]),
    ("trident_video_submit_planes", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("trident_video_submit_jpeg", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32]),
    ("trident_video_set_quality", C.c_int, [C.c_void_p, C.c_uint32]),
    ("trident_video_set_restart_interval", C.c_int, [C.c_void_p, C.c_uint32]),
    ("trident_video_end", C.c_int, [C.c_void_p]),
    ("trident_video_state", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    ("trident_video_convert_rgba", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    ("trident_app_set_dataset_capture", C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_uint32]),
    ("trident_app_dataset_capture_state", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.c_char_p,
                                                    C.c_uint32]),
    ("trident_app_set_ai_readback", C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]),
    ("trident_app_ai_readback_state", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("trident_app_acquire_frame", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    ("trident_app_readback_device_tensor", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32),
                                                     C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    ("trident_app_submit_ai_output", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int64), C.c_uint32]),
    ("trident_ai_normalise_output", C.c_int, [C.c_void_p, C.c_uint64, C.c_int64]),
    ("trident_app_load_ai_model", C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint32]),
    ("trident_app_resolve_ai_model_path", C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_int)]),
    ("trident_app_try_initialise_ai_model", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("trident_app_ai_debug_stats", C.c_int, [C.c_void_p, C.c_void_p]),
    ("trident_app_ai_model_info", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64 * 4), C.POINTER(C.c_int64 * 4)]),
    ("trident_app_finish_ai_inference", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]),
    ("trident_app_read_ai_blend_frame", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32),
                                                  C.POINTER(C.c_uint32)]),
    ("trident_dataset_create", C.c_int, [C.POINTER(C.c_void_p)]),
    ("trident_dataset_destroy", None, [C.c_void_p]),
    ("trident_dataset_set_directory", C.c_int, [C.c_void_p, C.c_char_p]),
    ("trident_dataset_set_interval", C.c_int, [C.c_void_p, C.c_uint32]),
    ("trident_dataset_enable", C.c_int, [C.c_void_p, C.c_int]),
    ("trident_dataset_reset", C.c_int, [C.c_void_p]),
    ("trident_dataset_record_input", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                               C.POINTER(C.c_int64), C.c_uint32]),
    ("trident_dataset_record_output", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int64), C.c_uint32]),
    ("trident_dataset_flush", C.c_int, [C.c_void_p]),
    ("trident_dataset_state", C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64)]),
    ("trident_dataset_write_npy", C.c_int, [C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_int64), C.c_uint32]),
    ("trident_app_set_entity_id_output", C.c_int, [C.c_void_p, C.c_uint32, C.c_int]),
    ("trident_app_pick_entity", C.c_int, [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.c_int),
                                          C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    ("trident_app_pick_entities_in_rect", C.c_int, [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                    C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_app_read_entity_ids", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32]),
    ("trident_app_set_selected_entity", C.c_int, [C.c_void_p, C.c_uint32]),
    ("trident_app_set_selection_outline", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float * 4), C.c_uint32]),
    ("trident_app_set_motion_vector_output", C.c_int, [C.c_void_p, C.c_uint32, C.c_int]),
    ("trident_app_read_motion_vectors", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    ("trident_app_motion_texture", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(abi.TriImage)]),
    ("trident_app_set_history_reprojection", C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_float]),
    ("trident_app_read_reprojection", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("trident_app_reprojection_textures", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(abi.TriImage), C.POINTER(abi.TriImage)]),
    ("trident_app_set_temporal_anti_aliasing", C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_uint32, C.c_int]),
    ("trident_app_is_temporal_anti_aliasing", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]),
    ("trident_app_read_resolved", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("trident_app_resolved_texture", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(abi.TriImage)]),
    ("trident_app_set_temporal_upscaling", C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_int]),
    ("trident_app_is_temporal_upscaling", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]),
    ("trident_app_read_upscaled", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("trident_app_upscaled_texture", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(abi.TriImage)]),
    ("trident_app_submit_text", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float * 2), C.POINTER(C.c_float * 4),
                                          C.c_char_p, C.c_uint32]),
    ("trident_app_set_font", C.c_int, [C.c_void_p, C.c_char_p, C.c_float]),
    ("trident_font_create", C.c_int, [C.POINTER(C.c_void_p)]),
    ("trident_font_destroy", None, [C.c_void_p]),
    ("trident_font_load", C.c_int, [C.c_void_p, C.c_char_p, C.c_float]),
    ("trident_font_load_memory", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float]),
    ("trident_font_atlas", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("trident_font_glyph", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float * 9)]),
    ("trident_font_metrics", C.c_int, [C.c_void_p, C.POINTER(C.c_float * 3)]),
    ("trident_font_layout", C.c_int, [C.c_void_p, C.POINTER(C.c_float * 2), C.POINTER(C.c_float * 4), C.c_char_p,
                                      C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_app_set_entity_animation", C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_float,
                                                   C.c_float, C.c_int, C.c_int]),
    ("trident_app_update_animation", C.c_int, [C.c_void_p, C.c_float]),
    ("trident_app_initialise_pose", C.c_int, [C.c_void_p, C.c_uint32]),
    ("trident_app_set_entity_state_machine", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64]),
    ("trident_app_entity_pose", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_app_entity_animation_state", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_int),
                                                     C.POINTER(C.c_uint64 * 3)]),
    ("trident_app_set_device_pose", C.c_int, [C.c_void_p, C.c_int]),
    ("trident_app_bone_palette_uploads", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("trident_anim_decompose", C.c_int, [C.c_void_p, C.POINTER(C.c_float * 10)]),
    ("trident_anim_register", C.c_int, [C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p),
                                        C.c_int32, C.POINTER(C.c_uint64)]),
    ("trident_anim_add_clip", C.c_int, [C.c_uint64, C.c_char_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p),
                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.POINTER(C.c_uint32)]),
    ("trident_anim_load", C.c_int, [C.c_char_p, C.POINTER(C.c_uint64)]),
    ("trident_anim_describe", C.c_int, [C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("trident_anim_clip_index", C.c_int, [C.c_uint64, C.c_char_p, C.POINTER(C.c_uint32)]),
    ("trident_anim_resolve_channels", C.c_int, [C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_anim_evaluate", C.c_int, [C.c_uint64, C.c_uint32, C.c_float, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_anim_advance", C.c_int, [C.c_uint64, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float,
                                       C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    ("trident_anim_eval_program", C.c_int, [C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                            C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_node_clip", C.c_int, [C.c_uint32, C.c_int, C.c_float, C.c_char_p, C.POINTER(C.c_uint64)]),
    ("trident_node_blend", C.c_int, [C.c_uint64, C.c_uint64, C.c_float, C.c_char_p, C.POINTER(C.c_uint64)]),
    ("trident_node_blend_space", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.c_char_p, C.POINTER(C.c_uint64)]),
    ("trident_node_destroy", C.c_int, [C.c_uint64]),
    ("trident_sm_create", C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("trident_sm_destroy", C.c_int, [C.c_uint64]),
    ("trident_sm_set_handles", C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64]),
    ("trident_sm_parameter", C.c_int, [C.c_uint64, C.c_char_p, C.c_int, C.c_float, C.c_int]),
    ("trident_sm_get_parameter", C.c_int, [C.c_uint64, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    ("trident_sm_add_layer", C.c_int, [C.c_uint64, C.c_char_p, C.c_float, C.c_int, C.POINTER(C.c_uint32)]),
    ("trident_sm_set_layer_mask", C.c_int, [C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32]),
    ("trident_sm_set_layer_weight", C.c_int, [C.c_uint64, C.c_uint32, C.c_float]),
    ("trident_sm_set_layer_entry", C.c_int, [C.c_uint64, C.c_uint32, C.c_char_p]),
    ("trident_sm_add_state", C.c_int, [C.c_uint64, C.c_uint32, C.c_char_p, C.c_uint64]),
    ("trident_sm_add_transition", C.c_int, [C.c_uint64, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, C.c_float, C.c_float,
                                            C.c_void_p, C.c_uint32]),
    ("trident_sm_update", C.c_int, [C.c_uint64, C.c_float]),
    ("trident_sm_pose", C.c_int, [C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_sm_program", C.c_int, [C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("trident_sm_program_mask", C.c_int, [C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("trident_sm_layer_state", C.c_int, [C.c_uint64, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_float),
                                         C.POINTER(C.c_float), C.POINTER(C.c_float)]),
]

class AiDebugStats(C.Structure):  # trident_ai_debug_stats
    _fields_ = [("model_initialised", C.c_int32), ("pending_job_count", C.c_uint32),
                ("completed_inference_count", C.c_uint64), ("last_inference_ms", C.c_double),
                ("average_inference_ms", C.c_double), ("texture_ready", C.c_int32), ("blend_strength", C.c_float),
                ("texture_width", C.c_uint32), ("texture_height", C.c_uint32), ("reserved_metric", C.c_double)]


_lib = None


def load_library(path=LIB_PATH):
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"Trident renderer shim not built: {path} (run __graft_entry__.build())")
    lib = C.CDLL(path)
    for name, res, args in _APP_FUNCTIONS:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc, what):
    if rc != abi.TRI_OK:
        raise TriError(rc, what)


def _vec(v):
    return None if v is None else (C.c_float * len(v))(*[float(x) for x in v])


class TridentApp:
    """One Renderer + ECS registry + editor/runtime cameras (Forge's ApplicationLayer, reduced)."""

    def __init__(self, raster_flags=0):
        self._lib = load_library()
        h = C.c_void_p()
        _check(self._lib.trident_app_create(raster_flags, C.byref(h)), "trident_app_create")
        self._h = h

    def close(self):
        if self._h:
            self._lib.trident_app_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append_mesh(self, vertices, indices, base_color=(1, 1, 1, 1), metallic=1.0, roughness=1.0, texture=None):
        v = np.ascontiguousarray(vertices, abi.VERTEX_DTYPE)
        i = np.ascontiguousarray(indices, np.uint32)
        out = C.c_uint32()
        _check(self._lib.trident_app_append_mesh(self._h, v.ctypes.data, v.shape[0], i.ctypes.data, i.size,
                                                 _vec(base_color), metallic, roughness,
                                                 texture.encode() if texture else None, C.byref(out)),
               "append_mesh")
        return out.value

    def upload_texture(self, path, rgba):
        rgba = np.ascontiguousarray(rgba, np.uint8)
        _check(self._lib.trident_app_upload_texture(self._h, path.encode(), rgba.ctypes.data, rgba.shape[1],
                                                    rgba.shape[0]), "upload_texture")

    def add_mesh_entity(self, primitive="none", mesh_index=0, position=(0, 0, 0), rotation=(0, 0, 0), scale=(1, 1, 1)):
        e = C.c_uint32()
        _check(self._lib.trident_app_add_mesh_entity(self._h, PRIMITIVE[primitive], mesh_index, _vec(position),
                                                     _vec(rotation), _vec(scale), C.byref(e)), "add_mesh_entity")
        return e.value

    def add_sprite_entity(self, position=(0, 0, 0), rotation=(0, 0, 0), scale=(1, 1, 1), tint=(1, 1, 1, 1),
                          uv_scale=(1, 1), uv_offset=(0, 0), tiling=1.0):
        """Transform + SpriteComponent (drawn after the meshes, Renderer.cpp:2996-3089)."""
        f = lambda v: (C.c_float * len(v))(*[float(x) for x in v])  # noqa: E731
        e = C.c_uint32()
        _check(self._lib.trident_app_add_sprite_entity(self._h, f(position), f(rotation), f(scale), f(tint), f(uv_scale),
                                                       f(uv_offset), float(tiling), C.byref(e)), "add_sprite_entity")
        return e.value

    def set_sprite_visible(self, entity, visible):
        _check(self._lib.trident_app_set_sprite_visible(self._h, entity, 1 if visible else 0), "set_sprite_visible")

    def entity_sprite(self, entity):
        """SpriteComponent: {tint, uv_scale, uv_offset, tiling, visible}, or None."""
        out = (C.c_float * 10)()
        if self._lib.trident_app_entity_sprite(self._h, entity, C.byref(out)) != 0:
            return None
        v = list(out)
        return {"tint": tuple(v[0:4]), "uv_scale": tuple(v[4:6]), "uv_offset": tuple(v[6:8]), "tiling": v[8],
                "visible": bool(v[9])}

    def set_entity_texture(self, entity, path):
        _check(self._lib.trident_app_set_entity_texture(self._h, entity, path.encode()), "set_entity_texture")

    def set_entity_transform(self, entity, position=None, rotation=None, scale=None):
        _check(self._lib.trident_app_set_entity_transform(self._h, entity, _vec(position), _vec(rotation), _vec(scale)),
               "set_entity_transform")

    def set_entity_visible(self, entity, visible):
        _check(self._lib.trident_app_set_entity_visible(self._h, entity, 1 if visible else 0), "set_entity_visible")

    def set_assets_dir(self, directory):
        """Renderer::SetAssetsDirectory (skybox discovery under directory/Skyboxes); returns the source."""
        buf = C.create_string_buffer(64)
        _check(self._lib.trident_app_set_assets_dir(self._h, os.fsencode(directory), buf, 64), "set_assets_dir")
        return buf.value.decode()

    def set_light_shadow_caster(self, entity, caster=True):
        _check(self._lib.trident_app_set_light_shadow_caster(self._h, entity, 1 if caster else 0), "shadow caster")

    def set_shadow_map_size(self, size):
        _check(self._lib.trident_app_set_shadow_map_size(self._h, size), "shadow map size")

    def set_device_count(self, count, devices=None):
        """Renderer::SetDeviceCount: viewports as `count` row bands on `devices` (tri_group), count <= 1: one context."""
        arr = (C.c_int32 * len(devices))(*devices) if devices else None
        _check(self._lib.trident_app_set_device_count(self._h, count, arr), "device count")

    def shadow_config(self):
        """The pre-pass configuration DrawFrame would use now (abi.TriShadowConfig), or None."""
        cfg, on = abi.TriShadowConfig(), C.c_int()
        _check(self._lib.trident_app_shadow_config(self._h, C.byref(cfg), C.byref(on)), "shadow_config")
        return cfg if on.value else None

    def viewport_texture(self, viewport_id):
        """Renderer::GetViewportTexture: the viewport's abi.TriImage handle."""
        img = abi.TriImage()
        _check(self._lib.trident_app_viewport_texture(self._h, viewport_id, C.byref(img)), "viewport_texture")
        return img

    def geometry_uploads(self):
        n = C.c_uint64()
        _check(self._lib.trident_app_geometry_uploads(self._h, C.byref(n)), "geometry_uploads")
        return n.value

    def set_entity_bones(self, entity, matrices):
        """AnimationComponent::m_BoneMatrices: float32 [n, 4, 4] column-major mat4s (m[col][row])."""
        m = np.ascontiguousarray(matrices, dtype=np.float32).reshape(-1, 16)
        _check(self._lib.trident_app_set_entity_bones(self._h, entity, m.ctypes.data if m.size else None,
                                                      m.shape[0]), "set_entity_bones")

    def set_entities_bones(self, entities, matrices):
        """set_entity_bones for many entities in one call: matrices float32 [entities, n, 16]."""
        e = np.ascontiguousarray(entities, np.uint32)
        m = np.ascontiguousarray(matrices, np.float32).reshape(e.size, -1, 16)
        _check(self._lib.trident_app_set_entities_bones(self._h, e.ctypes.data if e.size else None, e.size,
                                                        m.ctypes.data if m.size else None, m.shape[1]), "set_entities_bones")

    def set_entity_animation(self, entity, skeleton=None, animation=None, clip=None, time=0.0, speed=1.0, looping=True,
                             playing=True):
        """The playback fields of the entity's AnimationComponent (asset ids as given to anim_register)."""
        enc = lambda s: None if s is None else s.encode()  # noqa: E731
        _check(self._lib.trident_app_set_entity_animation(self._h, entity, enc(skeleton), enc(animation), enc(clip), time,
                                                          speed, int(looping), int(playing)), "set_entity_animation")

    def update_animation(self, dt):
        """ECS::AnimationSystem::Update."""
        _check(self._lib.trident_app_update_animation(self._h, dt), "update_animation")

    def set_entity_state_machine(self, entity, machine):
        """AnimationComponent::m_StateMachine: a StateMachine, or None to remove it."""
        _check(self._lib.trident_app_set_entity_state_machine(self._h, entity, machine.id if machine is not None else 0),
               "set_entity_state_machine")

    def initialise_pose(self, entity):
        _check(self._lib.trident_app_initialise_pose(self._h, entity), "initialise_pose")

    def entity_pose(self, entity):
        """The entity's bone matrices, float32 [n, 16] (device mode: evaluated on the CPU on demand)."""
        n = C.c_uint32()
        _check(self._lib.trident_app_entity_pose(self._h, entity, None, 0, C.byref(n)), "entity_pose")
        out = np.empty((n.value, 16), np.float32)
        _check(self._lib.trident_app_entity_pose(self._h, entity, out.ctypes.data if n.value else None, n.value,
                                                 C.byref(n)), "entity_pose")
        return out

    def entity_animation_state(self, entity):
        """(time, playing, skeleton handle, animation handle, clip index); an invalid handle or index is None."""
        t, p, h = C.c_float(), C.c_int(), (C.c_uint64 * 3)()
        _check(self._lib.trident_app_entity_animation_state(self._h, entity, C.byref(t), C.byref(p), C.byref(h)),
               "entity_animation_state")
        return (t.value, bool(p.value)) + tuple(None if v == ANIM_NO_HANDLE else v for v in h)

    def set_device_pose(self, enabled):
        """Renderer::SetDevicePoseEnabled; the animation system then only advances time."""
        _check(self._lib.trident_app_set_device_pose(self._h, int(enabled)), "set_device_pose")

    def bone_palette_uploads(self):
        n = C.c_uint64()
        _check(self._lib.trident_app_bone_palette_uploads(self._h, C.byref(n)), "bone_palette_uploads")
        return n.value

    def add_light(self, type, position=(0, 0, 0), direction=(-0.5, -1.0, -0.3), color=(1.0, 0.98, 0.92),
                  intensity=5.0, range=10.0, enabled=True):
        e = C.c_uint32()
        _check(self._lib.trident_app_add_light(self._h, LIGHT[type], _vec(position), _vec(direction), _vec(color),
                                               intensity, range, 1 if enabled else 0, C.byref(e)), "add_light")
        return e.value

    def set_camera(self, which, position, rotation=(0, 0, 0), fov=60.0, near=0.1, far=1000.0, ready=True):
        _check(self._lib.trident_app_set_camera(self._h, {"editor": 0, "runtime": 1}[which], _vec(position),
                                                _vec(rotation), fov, near, far, 1 if ready else 0), "set_camera")

    def set_viewport(self, viewport_id, width, height):
        _check(self._lib.trident_app_set_viewport(self._h, viewport_id, width, height), "set_viewport")

    def set_clear_color(self, rgba):
        _check(self._lib.trident_app_set_clear_color(self._h, _vec(rgba)), "set_clear_color")

    def set_skybox(self, faces):
        f = np.ascontiguousarray(faces, np.uint8)
        _check(self._lib.trident_app_set_skybox(self._h, f.ctypes.data, f.shape[1]), "set_skybox")

    def submit_text(self, viewport_id, position, color, text):
        """Renderer::SubmitText: text (str, encoded as UTF-8, or bytes as they are) for the viewport's next frame."""
        data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        pos, col = (C.c_float * 2)(*position), (C.c_float * 4)(*color)
        _check(self._lib.trident_app_submit_text(self._h, viewport_id, C.byref(pos), C.byref(col), data, len(data)),
               "submit_text")

    # ---- entity ids ----
    NO_ENTITY = 0xFFFFFFFF

    def set_entity_id_output(self, viewport_id, enabled=True):
        """Renderer::SetEntityIdOutputEnabled."""
        _check(self._lib.trident_app_set_entity_id_output(self._h, viewport_id, 1 if enabled else 0), "set_entity_id_output")

    def pick_entity(self, viewport_id, x, y):
        """Renderer::PickEntity: (entity, depth in [0, 1]), or None where it returns false."""
        hit, ent, z = C.c_int(), C.c_uint32(), C.c_float()
        _check(self._lib.trident_app_pick_entity(self._h, viewport_id, int(x), int(y), C.byref(hit), C.byref(ent), C.byref(z)),
               "pick_entity")
        return (ent.value, z.value) if hit.value else None

    def pick_entities_in_rect(self, viewport_id, x0, y0, x1, y1, capacity=1024):
        """Renderer::PickEntitiesInRect: the distinct entities, in draw order."""
        out = np.zeros(capacity, np.uint32)
        n = C.c_uint32()
        _check(self._lib.trident_app_pick_entities_in_rect(self._h, viewport_id, int(x0), int(y0), int(x1), int(y1),
                                                           out.ctypes.data, capacity, C.byref(n)), "pick_entities_in_rect")
        assert n.value <= capacity
        return out[: n.value].tolist()

    def read_entity_ids(self, viewport_id, width, height, background=0xFFFFFFFF):
        """Renderer::ReadViewportEntityIds: uint32 [height, width], or None where it returns false."""
        out = np.zeros((height, width), np.uint32)
        rc = self._lib.trident_app_read_entity_ids(self._h, viewport_id, out.ctypes.data, out.size, background)
        if rc == abi.TRI_E_STATE:
            return None
        _check(rc, "read_entity_ids")
        return out

    def set_selected_entity(self, entity):
        """Renderer::SetSelectedEntity (None: no selection)."""
        _check(self._lib.trident_app_set_selected_entity(self._h, self.NO_ENTITY if entity is None else entity),
               "set_selected_entity")

    def set_selection_outline(self, enabled, colour=(1.0, 0.6, 0.0, 1.0), width_px=2):
        """Renderer::SetSelectionOutline; False where the renderer refuses it."""
        col = (C.c_float * 4)(*[float(c) for c in colour])
        rc = self._lib.trident_app_set_selection_outline(self._h, 1 if enabled else 0, C.byref(col), width_px)
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, "set_selection_outline")
        return rc == abi.TRI_OK

    # ---- motion vectors ----
    def set_motion_vector_output(self, viewport_id, enabled=True):
        """Renderer::SetMotionVectorOutputEnabled; False where the renderer refuses it (SetDeviceCount > 1)."""
        rc = self._lib.trident_app_set_motion_vector_output(self._h, viewport_id, 1 if enabled else 0)
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, "set_motion_vector_output")
        return rc == abi.TRI_OK

    def read_motion_vectors(self, viewport_id, width, height):
        """Renderer::ReadViewportMotionVectors: float32 [height, width, 2], or None where it returns false."""
        out = np.zeros((height, width, 2), np.float32)
        rc = self._lib.trident_app_read_motion_vectors(self._h, viewport_id, out.ctypes.data, out.size)
        if rc == abi.TRI_E_STATE:
            return None
        _check(rc, "read_motion_vectors")
        return out

    def motion_texture(self, viewport_id):
        """Renderer::GetViewportMotionTexture: the motion image's abi.TriImage handle, or None."""
        img = abi.TriImage()
        rc = self._lib.trident_app_motion_texture(self._h, viewport_id, C.byref(img))
        if rc == abi.TRI_E_STATE:
            return None
        _check(rc, "motion_texture")
        return img

    # ---- history reprojection ----
    def set_history_reprojection(self, viewport_id, enabled=True, depth_tolerance=0.0):
        """Renderer::SetHistoryReprojectionEnabled; False where the renderer refuses it (SetDeviceCount > 1, a bad
        tolerance)."""
        rc = self._lib.trident_app_set_history_reprojection(self._h, viewport_id, 1 if enabled else 0, depth_tolerance)
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, "set_history_reprojection")
        return rc == abi.TRI_OK

    def read_reprojection(self, viewport_id, width, height):
        """Renderer::ReadViewportReprojection: (warped uint8 [height, width, 4] B G R A, mask uint8 [height, width]), or
        None where it returns false."""
        col = np.zeros((height, width, 4), np.uint8)
        mask = np.zeros((height, width), np.uint8)
        rc = self._lib.trident_app_read_reprojection(self._h, viewport_id, col.ctypes.data, mask.ctypes.data, mask.size)
        if rc == abi.TRI_E_STATE:
            return None
        _check(rc, "read_reprojection")
        return col, mask

    def reprojection_textures(self, viewport_id):
        """Renderer::GetViewportReprojectedTexture and GetViewportDisocclusionTexture: (colour, mask) abi.TriImage
        handles, or None."""
        col, mask = abi.TriImage(), abi.TriImage()
        rc = self._lib.trident_app_reprojection_textures(self._h, viewport_id, C.byref(col), C.byref(mask))
        if rc == abi.TRI_E_STATE:
            return None
        _check(rc, "reprojection_textures")
        return col, mask

    # ---- temporal anti-aliasing ----
    def set_temporal_anti_aliasing(self, viewport_id, enabled=True, alpha=0.1, period=8, reject_ids=True):
        """Renderer::SetTemporalAntiAliasingEnabled; False where the renderer refuses it (SetDeviceCount > 1, a bad alpha
        or period)."""
        rc = self._lib.trident_app_set_temporal_anti_aliasing(self._h, viewport_id, 1 if enabled else 0, alpha, period,
                                                              1 if reject_ids else 0)
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, "set_temporal_anti_aliasing")
        return rc == abi.TRI_OK

    def is_temporal_anti_aliasing(self, viewport_id):
        """Renderer::IsTemporalAntiAliasingEnabled."""
        on = C.c_int()
        _check(self._lib.trident_app_is_temporal_anti_aliasing(self._h, viewport_id, C.byref(on)), "is_temporal_anti_aliasing")
        return bool(on.value)

    def read_resolved(self, viewport_id, width, height):
        """Renderer::ReadViewportResolvedPixels and ReadViewportTaaMask: (resolved uint8 [height, width, 4] R G B A, mask
        uint8 [height, width]), or None where they return false."""
        col = np.zeros((height, width, 4), np.uint8)
        mask = np.zeros((height, width), np.uint8)
        rc = self._lib.trident_app_read_resolved(self._h, viewport_id, col.ctypes.data, mask.ctypes.data, mask.size)
        if rc == abi.TRI_E_STATE:
            return None
        _check(rc, "read_resolved")
        return col, mask

    def resolved_texture(self, viewport_id):
        """Renderer::GetViewportResolvedTexture: an abi.TriImage handle, or None."""
        img = abi.TriImage()
        rc = self._lib.trident_app_resolved_texture(self._h, viewport_id, C.byref(img))
        if rc == abi.TRI_E_STATE:
            return None
        _check(rc, "resolved_texture")
        return img

    # ---- temporal upscaling ----
    def set_temporal_upscaling(self, viewport_id, enabled=True, render_scale=0.5, alpha=0.1, reject_ids=True):
        """Renderer::SetTemporalUpscalingEnabled; False where the renderer refuses it (SetDeviceCount > 1, a bad scale
        or alpha, temporal anti-aliasing on for the viewport)."""
        rc = self._lib.trident_app_set_temporal_upscaling(self._h, viewport_id, 1 if enabled else 0, render_scale, alpha,
                                                          1 if reject_ids else 0)
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, "set_temporal_upscaling")
        return rc == abi.TRI_OK

    def is_temporal_upscaling(self, viewport_id):
        """Renderer::IsTemporalUpscalingEnabled."""
        on = C.c_int()
        _check(self._lib.trident_app_is_temporal_upscaling(self._h, viewport_id, C.byref(on)), "is_temporal_upscaling")
        return bool(on.value)

    def read_upscaled(self, viewport_id, width, height):
        """Renderer::ReadViewportUpscaledPixels and ReadViewportUpscaleMask at the viewport's full size: (uint8 [height,
        width, 4] R G B A, mask uint8 [height, width]), or None where they return false."""
        col = np.zeros((height, width, 4), np.uint8)
        mask = np.zeros((height, width), np.uint8)
        rc = self._lib.trident_app_read_upscaled(self._h, viewport_id, col.ctypes.data, mask.ctypes.data, mask.size)
        if rc == abi.TRI_E_STATE:
            return None
        _check(rc, "read_upscaled")
        return col, mask

    def upscaled_texture(self, viewport_id):
        """Renderer::GetViewportUpscaledTexture: an abi.TriImage handle, or None."""
        img = abi.TriImage()
        rc = self._lib.trident_app_upscaled_texture(self._h, viewport_id, C.byref(img))
        if rc == abi.TRI_E_STATE:
            return None
        _check(rc, "upscaled_texture")
        return img

    def set_font(self, path, pixel_height=32.0):
        """Renderer::SetTextFont; returns its bool."""
        rc = self._lib.trident_app_set_font(self._h, os.fsencode(path), pixel_height)
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, "set_font")
        return rc == abi.TRI_OK

    def draw_frame(self):
        _check(self._lib.trident_app_draw_frame(self._h), "draw_frame")

    def set_frames_in_flight(self, n):
        """Renderer::SetFramesInFlight (1 = the reference's pacing: DrawFrame waits for the previous frame)."""
        _check(self._lib.trident_app_set_frames_in_flight(self._h, n), "set_frames_in_flight")

    def finish_frame(self):
        """Wait for the last draw_frame's frame (Renderer::FinishFrame; the next draw_frame does it first)."""
        _check(self._lib.trident_app_finish_frame(self._h), "finish_frame")

    def set_recording(self, enabled, viewport_id=0, width=0, height=0, path=None):
        """Renderer::SetViewportRecordingEnabled -> (accepted, (width, height) of the recording extent)."""
        ext = (C.c_uint32 * 2)()
        rc = self._lib.trident_app_set_recording(self._h, 1 if enabled else 0, viewport_id, width, height,
                                                 os.fsencode(path) if path is not None else None, C.byref(ext))
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, "set_recording")
        return rc == abi.TRI_OK, (ext[0], ext[1])

    def set_recording_quality(self, quality):
        """Renderer::SetRecordingQuality -> GetRecordingQuality (the JPEG quality of .mkv recordings, clamped to 1..100)."""
        q = C.c_int()
        _check(self._lib.trident_app_set_recording_quality(self._h, quality, C.byref(q)), "set_recording_quality")
        return q.value

    def recording_state(self):
        """(Renderer::IsViewportRecording, GetRecordedFrameCount)."""
        rec, frames = C.c_int(), C.c_uint64()
        _check(self._lib.trident_app_recording_state(self._h, C.byref(rec), C.byref(frames)), "recording_state")
        return bool(rec.value), frames.value

    def read_pixels(self, viewport_id, width, height, depth=True):
        rgba = np.zeros((height, width, 4), np.uint8)
        d = np.zeros((height, width), np.float32) if depth else None
        _check(self._lib.trident_app_read_pixels(self._h, viewport_id, rgba.ctypes.data,
                                                 d.ctypes.data if depth else None), "read_pixels")
        return rgba, d

    def frame_inputs(self, viewport_id, capacity=4096):
        ubo = abi.TriGlobalUbo()
        draws = (abi.TriDraw * capacity)()
        n = C.c_uint32()
        _check(self._lib.trident_app_frame_inputs(self._h, viewport_id, C.byref(ubo), draws, capacity, C.byref(n)),
               "frame_inputs")
        return ubo, list(draws[: n.value])

    def geometry(self, capacity=4096):
        vp, ip = C.c_void_p(), C.c_void_p()
        nv, ni = C.c_size_t(), C.c_size_t()
        ranges = np.zeros(capacity, abi.MESH_RANGE_DTYPE)
        nr = C.c_uint32()
        _check(self._lib.trident_app_geometry(self._h, C.byref(vp), C.byref(nv), C.byref(ip), C.byref(ni),
                                              ranges.ctypes.data, capacity, C.byref(nr)), "geometry")
        vb = np.frombuffer((C.c_uint8 * (nv.value * abi.VERTEX_DTYPE.itemsize)).from_address(vp.value),
                           abi.VERTEX_DTYPE).copy() if nv.value else np.zeros(0, abi.VERTEX_DTYPE)
        ib = np.ctypeslib.as_array((C.c_uint32 * ni.value).from_address(ip.value)).copy() if ni.value else \
            np.zeros(0, np.uint32)
        return vb, ib, ranges[: nr.value].copy()

    def materials(self, capacity=1024):
        recs = (abi.TriMaterialRecord * capacity)()
        n = C.c_uint32()
        _check(self._lib.trident_app_materials(self._h, recs, capacity, C.byref(n)), "materials")
        return [(tuple(r.base_color_factor), tuple(r.material_factors)) for r in recs[: n.value]]

    def frame_timing(self):
        out = (C.c_double * 7)()
        _check(self._lib.trident_app_frame_timing(self._h, out), "frame_timing")
        keys = ("min_ms", "max_ms", "avg_ms", "min_fps", "max_fps", "avg_fps", "samples")
        return dict(zip(keys, list(out)))

    # ---- ingestion: ModelLoader + .trident scenes ----
    def import_model(self, path, capacity=4096):
        ents = (C.c_uint32 * capacity)()
        n = C.c_uint32()
        _check(self._lib.trident_app_import_model(self._h, str(path).encode(), ents, capacity, C.byref(n)),
               f"import_model({path})")
        return list(ents[: min(n.value, capacity)])

    def save_scene(self, path, name="Untitled"):
        _check(self._lib.trident_app_save_scene(self._h, str(path).encode(), name.encode()), "save_scene")

    def load_scene(self, path):
        n = C.c_uint32()
        _check(self._lib.trident_app_load_scene(self._h, str(path).encode(), C.byref(n)), f"load_scene({path})")
        return n.value

    def use_scene_camera(self):
        _check(self._lib.trident_app_use_scene_camera(self._h), "use_scene_camera")

    def entity_transform(self, entity):
        out = (C.c_float * 9)()
        _check(self._lib.trident_app_entity_transform(self._h, entity, out), "entity_transform")
        v = list(out)
        return tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:9])

    def entity_mesh(self, entity):
        out = (C.c_uint64 * 3)()
        _check(self._lib.trident_app_entity_mesh(self._h, entity, out), "entity_mesh")
        return {"mesh_index": out[0], "primitive": out[1], "source_mesh_index": out[2]}

    def entity_count(self):
        n = C.c_uint32()
        _check(self._lib.trident_app_entity_count(self._h, C.byref(n)), "entity_count")
        return n.value

    # ---- presentation: active viewport -> swapchain-sized image ----
    def set_present_extent(self, width, height):
        _check(self._lib.trident_app_set_present_extent(self._h, width, height), "set_present_extent")

    # ---- Default.frag's AI frame blend (SetAiBlendStrength / UploadAiInterpolationToGpu) ----
    def set_ai_blend_strength(self, strength):
        _check(self._lib.trident_app_set_ai_blend_strength(self._h, strength), "set_ai_blend_strength")

    def submit_ai_frame(self, pixels):
        """pixels: float32 [h, w, channels] in [0, 1] (the frame generator's output), or None to drop it."""
        if pixels is None:
            _check(self._lib.trident_app_submit_ai_frame(self._h, None, 0, 0, 0), "submit_ai_frame")
            return
        p = np.ascontiguousarray(pixels, np.float32)
        _check(self._lib.trident_app_submit_ai_frame(self._h, p.ctypes.data, p.shape[1], p.shape[0], p.shape[2]),
               "submit_ai_frame")

    def read_present(self, width, height):
        out = np.zeros((height, width, 4), np.uint8)
        _check(self._lib.trident_app_read_present(self._h, out.ctypes.data, width, height), "read_present")
        return out

    # ---- AI readback and dataset capture (the frame generator itself lives outside) ----
    def set_dataset_capture(self, enabled, directory=None, interval=0):
        """Renderer::SetFrameDatasetCaptureDirectory (unless None) / ...Interval (unless 0) / ...Enabled. Disabling
        returns once the queued samples are on disk."""
        _check(self._lib.trident_app_set_dataset_capture(self._h, 1 if enabled else 0,
                                                         os.fsencode(directory) if directory is not None else None,
                                                         interval), "set_dataset_capture")

    def dataset_capture_state(self):
        """(IsFrameDatasetCaptureEnabled, GetFrameDatasetCaptureDirectory, GetFrameDatasetCaptureInterval)."""
        en, iv, buf = C.c_int(), C.c_uint32(), C.create_string_buffer(4096)
        _check(self._lib.trident_app_dataset_capture_state(self._h, C.byref(en), C.byref(iv), buf, len(buf)),
               "dataset_capture_state")
        return bool(en.value), os.fsdecode(buf.value), iv.value

    def set_ai_readback(self, enabled, readback_ms=66, inference_ms=66):
        """Renderer::SetAiThrottleIntervals + SetAiReadbackEnabled -> accepted (False while SetDeviceCount > 1)."""
        rc = self._lib.trident_app_set_ai_readback(self._h, 1 if enabled else 0, readback_ms, inference_ms)
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, "set_ai_readback")
        return rc == abi.TRI_OK

    def ai_readback_enabled(self):
        en = C.c_int()
        _check(self._lib.trident_app_ai_readback_state(self._h, C.byref(en)), "ai_readback_state")
        return bool(en.value)

    def acquire_frame(self, out=None):
        """Renderer::TryAcquireRenderedFrame: float32 [h, w, 4] (R, G, B, A), or None when nothing is pending (or the
        inference throttle has not elapsed). `out`: a C-contiguous float32 array of at least h * w * 4 elements to
        fill instead of a new one (its first h * w * 4 elements are returned, shaped)."""
        w, h, got = C.c_uint32(), C.c_uint32(), C.c_int()
        # (a call without a buffer only reports the extent to size for; the tensor stays pending)
        rc = self._lib.trident_app_acquire_frame(self._h, None, 0, C.byref(w), C.byref(h), C.byref(got))
        if not (w.value and h.value):
            _check(rc, "acquire_frame")
            return None
        n = h.value * w.value * 4
        if out is None:
            out = np.empty(n, np.float32)
        if out.dtype != np.float32 or not out.flags.c_contiguous or out.size < n:
            raise ValueError("acquire_frame: out must be C-contiguous float32 with at least h * w * 4 elements")
        _check(self._lib.trident_app_acquire_frame(self._h, out.ctypes.data, out.size, C.byref(w), C.byref(h),
                                                   C.byref(got)), "acquire_frame")
        return out.reshape(-1)[:n].reshape(h.value, w.value, 4) if got.value else None

    def readback_device_tensor(self):
        """Renderer::GetFrameReadbackDeviceTensor: (device pointer, width, height) of the latest tensor, valid until
        the next draw_frame, or None."""
        p, w, h, got = C.c_void_p(), C.c_uint32(), C.c_uint32(), C.c_int()
        _check(self._lib.trident_app_readback_device_tensor(self._h, C.byref(p), C.byref(w), C.byref(h), C.byref(got)),
               "readback_device_tensor")
        return (p.value, w.value, h.value) if got.value else None

    # ---- the frame generator on the device ----
    def load_ai_model(self, path):
        """Renderer::LoadAiModel: raises TriError (TRI_E_INVALID, with the parser's message) for a damaged container."""
        buf = C.create_string_buffer(512)
        rc = self._lib.trident_app_load_ai_model(self._h, os.fsencode(path), buf, len(buf))
        if rc != abi.TRI_OK:
            raise TriError(rc, "load_ai_model: " + buf.value.decode(errors="replace"))

    def resolve_ai_model_path(self):
        """Renderer::ResolveAiModelPath: the path, or None."""
        buf, found = C.create_string_buffer(4096), C.c_int()
        _check(self._lib.trident_app_resolve_ai_model_path(self._h, buf, len(buf), C.byref(found)), "resolve_ai_model_path")
        return os.fsdecode(buf.value) if found.value else None

    def try_initialise_ai_model(self):
        ok = C.c_int()
        _check(self._lib.trident_app_try_initialise_ai_model(self._h, C.byref(ok)), "try_initialise_ai_model")
        return bool(ok.value)

    def ai_debug_stats(self):
        """Renderer::GetAiDebugStats as a dict."""
        s = AiDebugStats()
        _check(self._lib.trident_app_ai_debug_stats(self._h, C.byref(s)), "ai_debug_stats")
        return {name: getattr(s, name) for name, _ in AiDebugStats._fields_}

    def ai_model_info(self):
        """(initialised, input shape, output shape) of the frame generator."""
        ok, i, o = C.c_int(), (C.c_int64 * 4)(), (C.c_int64 * 4)()
        _check(self._lib.trident_app_ai_model_info(self._h, C.byref(ok), C.byref(i), C.byref(o)), "ai_model_info")
        return bool(ok.value), list(i), list(o)

    def finish_ai_inference(self, timeout_ms=5000):
        """Renderer::FinishAiInference: False when the deadline passed first."""
        ok = C.c_int()
        _check(self._lib.trident_app_finish_ai_inference(self._h, timeout_ms, C.byref(ok)), "finish_ai_inference")
        return bool(ok.value)

    def read_ai_blend_frame(self):
        """The active viewport's blend frame on the device, uint8 [h, w, 4] (R, G, B, A), or None without one."""
        w, h = C.c_uint32(), C.c_uint32()
        rc = self._lib.trident_app_read_ai_blend_frame(self._h, None, 0, C.byref(w), C.byref(h))
        if rc == abi.TRI_E_STATE:
            return None
        out = np.empty((h.value, w.value, 4), np.uint8)
        _check(self._lib.trident_app_read_ai_blend_frame(self._h, out.ctypes.data, out.size, C.byref(w), C.byref(h)),
               "read_ai_blend_frame")
        return out

    def submit_ai_output(self, data, shape):
        """Renderer::SubmitAiOutput: the generator's output (any float array) with its tensor shape -> accepted."""
        a = np.ascontiguousarray(data, np.float32)
        sh = (C.c_int64 * len(shape))(*[int(x) for x in shape]) if len(shape) else None
        rc = self._lib.trident_app_submit_ai_output(self._h, a.ctypes.data if a.size else None, a.size, sh, len(shape))
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, "submit_ai_output")
        return rc == abi.TRI_OK


class VideoEncoder:
    """Trident::VideoEncoder on its own (Y4M sessions on the host); every method returns the encoder's bool."""

    def __init__(self):
        self._lib = load_library()
        h = C.c_void_p()
        _check(self._lib.trident_video_create(C.byref(h)), "trident_video_create")
        self._h = h

    def close(self):
        if self._h:
            self._lib.trident_video_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _bool(self, rc, what):
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, what)
        return rc == abi.TRI_OK

    def begin(self, path, width, height, fps):
        return self._bool(self._lib.trident_video_begin(self._h, os.fsencode(path), width, height, fps), "video_begin")

    def submit_rgba(self, rgba, width, height):
        """SubmitFrame: RGBA8 rows (any array; its bytes are the pixel buffer, which may be empty)."""
        a = np.ascontiguousarray(rgba, np.uint8)
        return self._bool(self._lib.trident_video_submit_rgba(self._h, a.ctypes.data if a.size else None, a.size, width,
                                                              height), "video_submit_rgba")

    def submit_planes(self, yuv, width, height):
        a = np.ascontiguousarray(yuv, np.uint8)
        if a.size != 3 * width * height:
            raise ValueError("submit_planes: 3 * width * height bytes expected")
        return self._bool(self._lib.trident_video_submit_planes(self._h, a.ctypes.data, width, height),
                          "video_submit_planes")

    def submit_jpeg(self, jpeg, width, height):
        """SubmitJpeg: a complete JPEG (bytes or a uint8 array) into an .mkv session."""
        a = np.frombuffer(bytes(jpeg), np.uint8) if isinstance(jpeg, (bytes, bytearray)) else np.ascontiguousarray(jpeg, np.uint8)
        return self._bool(self._lib.trident_video_submit_jpeg(self._h, a.ctypes.data if a.size else None, a.size, width,
                                                              height), "video_submit_jpeg")

    def set_quality(self, quality):
        """SetQuality: False (unchanged) outside 1..100."""
        return self._lib.trident_video_set_quality(self._h, quality) == abi.TRI_OK

    def set_restart_interval(self, restart_mcus):
        """SetRestartInterval: False (unchanged) outside 0..65535."""
        return self._lib.trident_video_set_restart_interval(self._h, restart_mcus) == abi.TRI_OK

    def end(self):
        return self._bool(self._lib.trident_video_end(self._h), "video_end")

    def state(self):
        """(IsSessionActive, frames written)."""
        act, frames = C.c_int(), C.c_uint64()
        _check(self._lib.trident_video_state(self._h, C.byref(act), C.byref(frames)), "video_state")
        return bool(act.value), frames.value


class Font:
    """Trident::TextRenderer on its own (no app, no device): load a TrueType file, read the baked atlas, the glyph
    table and the metrics, lay a string out into tri_text_quad rows."""

    def __init__(self, path=None, pixel_height=32.0):
        self._lib = load_library()
        h = C.c_void_p()
        _check(self._lib.trident_font_create(C.byref(h)), "trident_font_create")
        self._h = h
        if path is not None and not self.load(path, pixel_height):
            raise ValueError(f"font {path} could not be loaded")

    def close(self):
        if self._h:
            self._lib.trident_font_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _bool(self, rc, what):
        if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
            _check(rc, what)
        return rc == abi.TRI_OK

    def load(self, path, pixel_height=32.0):
        return self._bool(self._lib.trident_font_load(self._h, os.fsencode(path), pixel_height), "font_load")

    def load_memory(self, data, pixel_height=32.0):
        a = np.frombuffer(bytes(data), np.uint8)
        if a.size == 0:
            return False
        return self._bool(self._lib.trident_font_load_memory(self._h, a.ctypes.data, a.size, pixel_height),
                          "font_load_memory")

    def atlas(self):
        """uint8 [height, width] coverage."""
        w, h = C.c_uint32(), C.c_uint32()
        _check(self._lib.trident_font_atlas(self._h, None, 0, C.byref(w), C.byref(h)), "font_atlas")
        out = np.empty((h.value, w.value), np.uint8)
        _check(self._lib.trident_font_atlas(self._h, out.ctypes.data, out.size, None, None), "font_atlas")
        return out

    def glyph(self, codepoint):
        """ResolveGlyph(codepoint): float32 (offset.x, offset.y, size.x, size.y, u0, v0, u1, v1, advance)."""
        out = (C.c_float * 9)()
        _check(self._lib.trident_font_glyph(self._h, codepoint, C.byref(out)), "font_glyph")
        return np.array(out[:], np.float32)

    def metrics(self):
        """(line advance, scale in pixels per font unit, pixel height)."""
        out = (C.c_float * 3)()
        _check(self._lib.trident_font_metrics(self._h, C.byref(out)), "font_metrics")
        return tuple(np.array(out[:], np.float32))

    def layout(self, text, position, color=(1.0, 1.0, 1.0, 1.0)):
        """float32 [n, 12] tri_text_quad rows of one string (str -> UTF-8, or bytes as they are)."""
        data = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        pos, col = (C.c_float * 2)(*position), (C.c_float * 4)(*color)
        out = np.zeros((max(len(data), 1), 12), np.float32)  # at most one quad per byte
        n = C.c_uint32()
        _check(self._lib.trident_font_layout(self._h, C.byref(pos), C.byref(col), data, len(data), out.ctypes.data,
                                             out.shape[0], C.byref(n)), "font_layout")
        return out[:n.value].copy()


class DatasetRecorder:
    """Trident::FrameDatasetRecorder on its own (no app, no device)."""

    def __init__(self):
        self._lib = load_library()
        h = C.c_void_p()
        _check(self._lib.trident_dataset_create(C.byref(h)), "trident_dataset_create")
        self._h = h

    def close(self):
        if self._h:
            self._lib.trident_dataset_destroy(self._h)  # (writes what is queued)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _shape(shape):
        shape = [] if shape is None else [int(x) for x in shape]
        return ((C.c_int64 * len(shape))(*shape) if shape else None), len(shape)

    def set_directory(self, directory):
        _check(self._lib.trident_dataset_set_directory(self._h, os.fsencode(directory)), "dataset_set_directory")

    def set_interval(self, interval):
        _check(self._lib.trident_dataset_set_interval(self._h, interval), "dataset_set_interval")

    def enable(self, enabled):
        _check(self._lib.trident_dataset_enable(self._h, 1 if enabled else 0), "dataset_enable")

    def reset(self):
        _check(self._lib.trident_dataset_reset(self._h), "dataset_reset")

    def record_input(self, data, width, height, channels, shape=None):
        a = np.ascontiguousarray(data, np.float32)
        sh, rank = self._shape(shape)
        _check(self._lib.trident_dataset_record_input(self._h, a.ctypes.data if a.size else None, a.size, width, height,
                                                      channels, sh, rank), "dataset_record_input")

    def record_output(self, data, shape=None):
        a = np.ascontiguousarray(data, np.float32)
        sh, rank = self._shape(shape)
        _check(self._lib.trident_dataset_record_output(self._h, a.ctypes.data if a.size else None, a.size, sh, rank),
               "dataset_record_output")

    def flush(self):
        _check(self._lib.trident_dataset_flush(self._h), "dataset_flush")

    def state(self):
        """(enabled, interval, next sample index, inputs waiting for an output)."""
        en, iv, nxt, pend = C.c_int(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(self._lib.trident_dataset_state(self._h, C.byref(en), C.byref(iv), C.byref(nxt), C.byref(pend)),
               "dataset_state")
        return bool(en.value), iv.value, nxt.value, pend.value


def write_npy(path, data, shape):
    """FrameDatasetRecorder::WriteNpyFile alone -> written (False: refused, no file)."""
    lib = load_library()
    a = np.ascontiguousarray(data, np.float32)
    sh, rank = DatasetRecorder._shape(shape)
    rc = lib.trident_dataset_write_npy(os.fsencode(path), a.ctypes.data if a.size else None, a.size, sh, rank)
    if rc not in (abi.TRI_OK, abi.TRI_E_STATE):
        _check(rc, "dataset_write_npy")
    return rc == abi.TRI_OK


def normalise_ai_output(data, channels):
    """Renderer::NormaliseAndReorderAiOutput on a copy: float32, flat."""
    lib = load_library()
    a = np.array(data, np.float32).reshape(-1)
    _check(lib.trident_ai_normalise_output(a.ctypes.data if a.size else None, a.size, channels), "ai_normalise_output")
    return a


def convert_rgba(rgba):
    """VideoEncoder::ConvertRgbaToYuv444 on the host: RGBA8 pixels [..., 4] -> uint8 [3, pixels] (Y, U, V planes)."""
    lib = load_library()
    a = np.ascontiguousarray(rgba, np.uint8).reshape(-1, 4)
    out = np.empty((3, a.shape[0]), np.uint8)
    _check(lib.trident_video_convert_rgba(a.ctypes.data, a.shape[0], out.ctypes.data), "video_convert_rgba")
    return out


def load_image(path, flip=True):
    """TextureLoader::Load (flip=True, 2D textures) or one cube face (flip=False): uint8 [h, w, 4] RGBA."""
    lib = load_library()
    w, h = C.c_uint32(), C.c_uint32()
    _check(lib.trident_load_image(os.fsencode(path), 1 if flip else 0, None, 0, C.byref(w), C.byref(h)), "load_image")
    out = np.empty((h.value, w.value, 4), np.uint8)
    _check(lib.trident_load_image(os.fsencode(path), 1 if flip else 0, out.ctypes.data, out.nbytes, C.byref(w),
                                  C.byref(h)), "load_image")
    return out


def load_default_skybox(assets_dir):
    """DiscoverDefaultSkybox (Renderer.cpp:3830-3927): (faces uint8 [6, n, n, 4] or None, source)."""
    lib = load_library()
    n = C.c_uint32()
    src = C.create_string_buffer(64)
    _check(lib.trident_load_default_skybox(os.fsencode(assets_dir), None, 0, C.byref(n), src, 64), "load_default_skybox")
    if n.value == 0:
        return None, src.value.decode()
    faces = np.empty((6, n.value, n.value, 4), np.uint8)
    _check(lib.trident_load_default_skybox(os.fsencode(assets_dir), faces.ctypes.data, faces.nbytes, C.byref(n), src, 64),
           "load_default_skybox")
    return faces, src.value.decode()


class CubemapInfo(C.Structure):  # trident_cubemap_info
    _fields_ = [("format", C.c_uint32), ("size", C.c_uint32), ("mip_count", C.c_uint32), ("bytes_per_pixel", C.c_uint32),
                ("is_hdr", C.c_uint32), ("region_levels", C.c_uint32), ("bytes", C.c_uint64)]


def _load_cubemap(call, what):
    """(info dict, the chain's bytes as uint8 [bytes]) or (None, None): `call(info, texels, capacity)` twice."""
    info = CubemapInfo()
    _check(call(C.byref(info), None, 0), what)
    if info.size == 0:
        return None, None
    texels = np.empty(info.bytes, np.uint8)
    _check(call(C.byref(info), texels.ctypes.data, texels.nbytes), what)
    return {k: getattr(info, k) for k, _ in CubemapInfo._fields_}, texels


def load_default_skybox_ex(assets_dir):
    """DiscoverDefaultSkybox for every cubemap it can return: (info, texels, source); info None when nothing valid."""
    lib = load_library()
    src = C.create_string_buffer(64)
    info, texels = _load_cubemap(lambda i, t, c: lib.trident_load_default_skybox_ex(os.fsencode(assets_dir), i, t, c, src, 64),
                                 "load_default_skybox_ex")
    return info, texels, src.value.decode()


def load_skybox_ktx(path):
    """SkyboxTextureLoader::LoadFromKtx: (info, texels), or (None, None) for a file it refuses."""
    lib = load_library()
    return _load_cubemap(lambda i, t, c: lib.trident_load_skybox(os.fsencode(path), 0, i, t, c), "load_skybox_ktx")


def load_skybox_directory(path):
    """SkyboxTextureLoader::LoadFromDirectory: (info, texels), or (None, None)."""
    lib = load_library()
    return _load_cubemap(lambda i, t, c: lib.trident_load_skybox(os.fsencode(path), 1, i, t, c), "load_skybox_directory")


def float_to_half(values):
    """Loader::FloatToHalf (the reference's routine: ties round away from zero) over float32 values -> uint16."""
    lib = load_library()
    v = np.ascontiguousarray(values, np.float32)
    out = np.empty(v.shape, np.uint16)
    _check(lib.trident_float_to_half(v.ctypes.data, out.ctypes.data, v.size), "float_to_half")
    return out


# ---- skeletal animation on the CPU (trident_anim_*): the asset service and the float32 player, no GPU ----
ANIM_NO_HANDLE = 0xFFFFFFFFFFFFFFFF
ANIM_NO_CLIP = 0xFFFFFFFF


def _names(names, n):
    if names is None:
        return None
    arr = (C.c_char_p * max(n, 1))()
    for i, s in enumerate(names):
        arr[i] = None if s is None else s.encode()
    return arr


def anim_decompose(local_bind):
    """Animation::DecomposeBindTransform: (translation [3], rotation [4] w x y z, scale [3]) as float32."""
    lib = load_library()
    m = np.ascontiguousarray(local_bind, np.float32).reshape(16)
    out = (C.c_float * 10)()
    _check(lib.trident_anim_decompose(m.ctypes.data, C.byref(out)), "anim_decompose")
    v = np.array(out[:], np.float32)
    return v[0:3], v[3:7], v[7:10]


def anim_register(asset_id, parents, local_binds, inverse_binds, source_names=None, root_index=-1):
    """RegisterRuntimeAsset of a skeleton (matrices [n, 16] column-major); returns the handle."""
    lib = load_library()
    p = np.ascontiguousarray(parents, np.int32).reshape(-1)
    lb = np.ascontiguousarray(local_binds, np.float32).reshape(-1, 16)
    ib = np.ascontiguousarray(inverse_binds, np.float32).reshape(-1, 16)
    assert lb.shape[0] == p.size == ib.shape[0]
    h = C.c_uint64()
    opt = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    _check(lib.trident_anim_register(asset_id.encode(), p.size, opt(p), opt(lb), opt(ib), _names(source_names, p.size),
                                     root_index, C.byref(h)), "anim_register")
    return h.value


def anim_add_clip(handle, name, duration, channels, vec_times, vec_values, quat_times, quat_values, stored_bones=None,
                  source_names=None):
    """Append a clip: channels are abi.POSE_CHANNEL_DTYPE rows over the vector / quaternion key arrays."""
    lib = load_library()
    ch = np.ascontiguousarray(channels, abi.POSE_CHANNEL_DTYPE)
    vt = np.ascontiguousarray(vec_times, np.float32).reshape(-1)
    vv = np.ascontiguousarray(vec_values, np.float32).reshape(-1, 3)
    qt = np.ascontiguousarray(quat_times, np.float32).reshape(-1)
    qv = np.ascontiguousarray(quat_values, np.float32).reshape(-1, 4)
    sb = None if stored_bones is None else np.ascontiguousarray(stored_bones, np.int32)
    opt = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
    out = C.c_uint32()
    _check(lib.trident_anim_add_clip(handle, name.encode(), duration, opt(ch), opt(sb), _names(source_names, ch.size),
                                     ch.size, opt(vt), opt(vv), vt.size, opt(qt), opt(qv), qt.size, C.byref(out)),
           "anim_add_clip")
    return out.value


def anim_load(path):
    """AnimationAssetService::AcquireSkeleton of a model file: the handle, or None when it yields no bones or clips."""
    lib = load_library()
    h = C.c_uint64()
    rc = lib.trident_anim_load(os.fsencode(path), C.byref(h))
    return h.value if rc == abi.TRI_OK else None


def anim_describe(handle):
    """The asset as a dict (trident_anim_describe's JSON)."""
    import json

    lib = load_library()
    n = C.c_uint64()
    _check(lib.trident_anim_describe(handle, None, 0, C.byref(n)), "anim_describe")
    buf = C.create_string_buffer(n.value)
    _check(lib.trident_anim_describe(handle, buf, n.value, C.byref(n)), "anim_describe")
    return json.loads(buf.value.decode())


def anim_clip_index(handle, name):
    """ResolveClipIndex, or None."""
    lib = load_library()
    out = C.c_uint32()
    rc = lib.trident_anim_clip_index(handle, name.encode(), C.byref(out))
    return out.value if rc == abi.TRI_OK else None


def anim_resolve_channels(handle, clip_index):
    lib = load_library()
    n = C.c_uint32()
    _check(lib.trident_anim_resolve_channels(handle, clip_index, None, 0, C.byref(n)), "anim_resolve_channels")
    out = np.empty(n.value, np.int32)
    _check(lib.trident_anim_resolve_channels(handle, clip_index, out.ctypes.data if n.value else None, n.value,
                                             C.byref(n)), "anim_resolve_channels")
    return out


def anim_evaluate(handle, clip_index, time):
    """The CPU player's pose at `time`: float32 [bones, 16] (clip_index None: the bind pose)."""
    lib = load_library()
    clip = ANIM_NO_CLIP if clip_index is None else clip_index
    n = C.c_uint32()
    _check(lib.trident_anim_evaluate(handle, clip, time, None, 0, C.byref(n)), "anim_evaluate")
    out = np.empty((n.value, 16), np.float32)
    _check(lib.trident_anim_evaluate(handle, clip, time, out.ctypes.data, n.value, C.byref(n)), "anim_evaluate")
    return out


def anim_eval_program(handle, ops, masks=()):
    """The CPU interpreter's matrices for a pose program: ops = rows of (op, a, f) or an abi.POSE_OP_DTYPE array (a CLIP's
    `a` indexes the asset's clips, a BLEND / ADD's `a` indexes `masks`, a sequence of weight arrays); float32 [bones, 16]."""
    lib = load_library()
    if isinstance(ops, np.ndarray) and ops.dtype == abi.POSE_OP_DTYPE:
        o = np.ascontiguousarray(ops)
    else:
        o = np.zeros(len(ops), abi.POSE_OP_DTYPE)
        for i, (op, a, f) in enumerate(ops):
            o[i] = (op, a, f, 0)
    counts = np.array([len(m) for m in masks], np.uint32)
    weights = np.concatenate([np.asarray(m, np.float32).reshape(-1) for m in masks]) if len(masks) else np.zeros(0, np.float32)
    weights = np.ascontiguousarray(weights, np.float32)
    opt = lambda a: a.ctypes.data if a.size else None  # noqa: E731
    n = C.c_uint32()
    args = (handle, opt(o), o.size, opt(weights), opt(counts), counts.size)
    _check(lib.trident_anim_eval_program(*args, None, 0, C.byref(n)), "anim_eval_program")
    out = np.empty((n.value, 16), np.float32)
    _check(lib.trident_anim_eval_program(*args, out.ctypes.data, n.value, C.byref(n)), "anim_eval_program")
    return out


def anim_advance(handle, clip_index, time, dt, speed=1.0, looping=True, playing=True):
    """AnimationPlayer::Update from the given state: (time, playing) afterwards."""
    lib = load_library()
    t, p = C.c_float(), C.c_int()
    _check(lib.trident_anim_advance(handle, ANIM_NO_CLIP if clip_index is None else clip_index, time, speed,
                                    int(looping), int(playing), dt, C.byref(t), C.byref(p)), "anim_advance")
    return t.value, bool(p.value)


# ---- animation state machines and blend trees (trident_sm_* / trident_node_*): host state only, no GPU ----
SM_FLOAT, SM_BOOL, SM_INTEGER, SM_TRIGGER = 0, 1, 2, 3
SM_COMPARISON = {"==": 0, "!=": 1, ">": 2, "<": 3, ">=": 4, "<=": 5, "triggered": 6}


class SmCondition(C.Structure):
    _fields_ = [("parameter", C.c_char_p), ("comparison", C.c_int32), ("float_value", C.c_float),
                ("int_value", C.c_int32), ("bool_value", C.c_int32)]


def _opt_name(name):
    return None if name is None else name.encode()


def node_clip(clip_index, looping=True, speed=1.0, speed_parameter=None):
    """A ClipNode's id (clip_index None: no clip)."""
    out = C.c_uint64()
    _check(load_library().trident_node_clip(ANIM_NO_CLIP if clip_index is None else clip_index, int(looping), speed,
                                            _opt_name(speed_parameter), C.byref(out)), "node_clip")
    return out.value


def node_blend(first, second, weight=0.5, weight_parameter=None):
    """A BlendNode's id over two node ids (None: no child); the children's ids are consumed."""
    out = C.c_uint64()
    _check(load_library().trident_node_blend(first or 0, second or 0, weight, _opt_name(weight_parameter), C.byref(out)),
           "node_blend")
    return out.value


def node_blend_space(samples, default=0.0, parameter=None):
    """A BlendSpace1DNode's id: samples = (clip index or None, position) pairs."""
    clips = np.array([ANIM_NO_CLIP if c is None else c for c, _ in samples], np.uint32)
    pos = np.array([p for _, p in samples], np.float32)
    out = C.c_uint64()
    _check(load_library().trident_node_blend_space(clips.ctypes.data if clips.size else None,
                                                   pos.ctypes.data if pos.size else None, clips.size, default,
                                                   _opt_name(parameter), C.byref(out)), "node_blend_space")
    return out.value


class StateMachine:
    """Animation::AnimationStateMachine on the shim's asset service (handles from anim_register; None: invalid)."""

    def __init__(self, skeleton_handle, library_handle=None):
        self._lib = load_library()
        out = C.c_uint64()
        lib_handle = skeleton_handle if library_handle is None else library_handle
        _check(self._lib.trident_sm_create(ANIM_NO_HANDLE if skeleton_handle is None else skeleton_handle,
                                           ANIM_NO_HANDLE if lib_handle is None else lib_handle, C.byref(out)), "sm_create")
        self.id = out.value

    def close(self):
        if self.id:
            self._lib.trident_sm_destroy(self.id)
            self.id = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_handles(self, skeleton_handle, library_handle):
        h = lambda v: ANIM_NO_HANDLE if v is None else v  # noqa: E731
        _check(self._lib.trident_sm_set_handles(self.id, h(skeleton_handle), h(library_handle)), "sm_set_handles")

    def add_parameter(self, name, kind, value=0.0):
        _check(self._lib.trident_sm_parameter(self.id, name.encode(), kind, float(value), 1), "sm_add_parameter")

    def set_parameter(self, name, kind, value):
        _check(self._lib.trident_sm_parameter(self.id, name.encode(), kind, float(value), 0), "sm_set_parameter")

    def fire(self, name):
        self.set_parameter(name, SM_TRIGGER, 1.0)

    def reset_trigger(self, name):
        self.set_parameter(name, SM_TRIGGER, 0.0)

    def parameter(self, name):
        """(type, AsFloat, trigger set) or None for a parameter the machine does not have."""
        t, f, trig = C.c_int(), C.c_float(), C.c_int()
        if self._lib.trident_sm_get_parameter(self.id, name.encode(), C.byref(t), C.byref(f), C.byref(trig)) != abi.TRI_OK:
            return None
        return t.value, f.value, bool(trig.value)

    def add_layer(self, name, weight=1.0, additive=False):
        out = C.c_uint32()
        _check(self._lib.trident_sm_add_layer(self.id, name.encode(), weight, int(additive), C.byref(out)), "sm_add_layer")
        return out.value

    def set_layer_mask(self, layer, weights):
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        _check(self._lib.trident_sm_set_layer_mask(self.id, layer, w.ctypes.data if w.size else None, w.size), "sm_set_layer_mask")

    def set_layer_weight(self, layer, weight):
        _check(self._lib.trident_sm_set_layer_weight(self.id, layer, weight), "sm_set_layer_weight")

    def set_layer_entry(self, layer, state):
        _check(self._lib.trident_sm_set_layer_entry(self.id, layer, state.encode()), "sm_set_layer_entry")

    def add_state(self, layer, name, root_node):
        _check(self._lib.trident_sm_add_state(self.id, layer, name.encode(), root_node or 0), "sm_add_state")

    def add_transition(self, layer, from_state, target_state, fade=0.2, exit_time=None, conditions=()):
        """conditions: (parameter, comparison in SM_COMPARISON, value) with value a bool, an int or a float."""
        arr = (SmCondition * max(len(conditions), 1))()
        for i, (name, cmp_, value) in enumerate(conditions):
            arr[i] = SmCondition(name.encode(), SM_COMPARISON[cmp_], float(value), int(value), int(bool(value)))
        _check(self._lib.trident_sm_add_transition(self.id, layer, from_state.encode(), target_state.encode(),
                                                   int(exit_time is not None), exit_time or 0.0, fade,
                                                   C.cast(arr, C.c_void_p) if conditions else None, len(conditions)),
               "sm_add_transition")

    def update(self, dt):
        _check(self._lib.trident_sm_update(self.id, dt), "sm_update")

    def pose(self):
        n = C.c_uint32()
        _check(self._lib.trident_sm_pose(self.id, None, 0, C.byref(n)), "sm_pose")
        out = np.empty((n.value, 16), np.float32)
        _check(self._lib.trident_sm_pose(self.id, out.ctypes.data if n.value else None, n.value, C.byref(n)), "sm_pose")
        return out

    def program(self):
        """(ops as (op, a, f) tuples, masks as float32 arrays) of the last update."""
        n, m = C.c_uint32(), C.c_uint32()
        _check(self._lib.trident_sm_program(self.id, None, 0, C.byref(n), C.byref(m)), "sm_program")
        ops = np.zeros(n.value, abi.POSE_OP_DTYPE)
        _check(self._lib.trident_sm_program(self.id, ops.ctypes.data if n.value else None, n.value, C.byref(n), C.byref(m)),
               "sm_program")
        masks = []
        for i in range(m.value):
            k = C.c_uint32()
            _check(self._lib.trident_sm_program_mask(self.id, i, None, 0, C.byref(k)), "sm_program_mask")
            w = np.zeros(k.value, np.float32)
            _check(self._lib.trident_sm_program_mask(self.id, i, w.ctypes.data if k.value else None, k.value, C.byref(k)),
                   "sm_program_mask")
            masks.append(w)
        return [(int(o["op"]), int(o["a"]), float(o["f"])) for o in ops], masks

    def layer_state(self, layer):
        """(current state name, next state name, time in state, transition elapsed, transition duration)."""
        cur, nxt = C.create_string_buffer(256), C.create_string_buffer(256)
        t, e, d = C.c_float(), C.c_float(), C.c_float()
        _check(self._lib.trident_sm_layer_state(self.id, layer, cur, nxt, 256, C.byref(t), C.byref(e), C.byref(d)),
               "sm_layer_state")
        return cur.value.decode(), nxt.value.decode(), t.value, e.value, d.value
