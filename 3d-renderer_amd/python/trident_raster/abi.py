"""ctypes / numpy mirrors of include/tri_raster.h (the C-ABI boundary).

Struct layouts are byte-identical to the reference's GPU ABI structs:
Vertex (Trident/src/Renderer/Vertex.h:9-78, 100 B), RenderablePushConstant (RenderData.h:14-30,
128 B), GlobalUniformBuffer (UniformBuffer.h:17-28, 480 B), MaterialUniformBuffer (32 B),
MeshDrawInfo (Renderer.h:293-299).
"""
import ctypes as C

import numpy as np

TRI_RASTER_ABI_VERSION = 2  # include/tri_raster.h

TRI_OK = 0
TRI_E_INVALID = -1
TRI_E_HIP = -2
TRI_E_OOM = -3
TRI_E_OVERFLOW = -4
TRI_E_UNSUPPORTED = -5
TRI_E_STATE = -6
TRI_E_TIMEOUT = -7

TRI_MAX_POINT_LIGHTS = 8
TRI_MAX_TEXTURE_SLOTS = 256
TRI_FLAG_NO_DEPTH_OUTPUT = 0x1
TRI_FLAG_EXACT_SHADING = 0x2
TRI_FLAG_CLUSTER_CULL = 0x4

VERTEX_DTYPE = np.dtype(
    [
        ("position", "<f4", 3),
        ("normal", "<f4", 3),
        ("tangent", "<f4", 3),
        ("bitangent", "<f4", 3),
        ("color", "<f4", 3),
        ("texcoord", "<f4", 2),
        ("bone_indices", "<i4", 4),
        ("bone_weights", "<f4", 4),
    ]
)
assert VERTEX_DTYPE.itemsize == 100

MESH_RANGE_DTYPE = np.dtype(
    [("first_index", "<u4"), ("index_count", "<u4"), ("base_vertex", "<i4"), ("material_index", "<i4")]
)


class TriVertex(C.Structure):
    _fields_ = [
        ("position", C.c_float * 3),
        ("normal", C.c_float * 3),
        ("tangent", C.c_float * 3),
        ("bitangent", C.c_float * 3),
        ("color", C.c_float * 3),
        ("texcoord", C.c_float * 2),
        ("bone_indices", C.c_int32 * 4),
        ("bone_weights", C.c_float * 4),
    ]


class TriMeshRange(C.Structure):
    _fields_ = [
        ("first_index", C.c_uint32),
        ("index_count", C.c_uint32),
        ("base_vertex", C.c_int32),
        ("material_index", C.c_int32),
    ]


class TriPushConstant(C.Structure):
    _fields_ = [
        ("model", C.c_float * 16),
        ("tint", C.c_float * 4),
        ("texture_scale", C.c_float * 2),
        ("texture_offset", C.c_float * 2),
        ("tiling_factor", C.c_float),
        ("texture_slot", C.c_int32),
        ("use_material_override", C.c_int32),
        ("sort_bias", C.c_float),
        ("material_index", C.c_int32),
        ("padding0", C.c_int32),
        ("bone_offset", C.c_int32),
        ("bone_count", C.c_int32),
    ]


class TriDraw(C.Structure):
    _fields_ = [("mesh_index", C.c_uint32), ("reserved", C.c_uint32 * 3), ("pc", TriPushConstant)]


class TriPointLight(C.Structure):
    _fields_ = [("position_range", C.c_float * 4), ("color_intensity", C.c_float * 4)]


class TriGlobalUbo(C.Structure):
    _fields_ = [
        ("view", C.c_float * 16),
        ("projection", C.c_float * 16),
        ("camera_position", C.c_float * 4),
        ("ambient_color_intensity", C.c_float * 4),
        ("directional_light_direction", C.c_float * 4),
        ("directional_light_color", C.c_float * 4),
        ("light_counts", C.c_uint32 * 4),
        ("ai_blend_config", C.c_float * 4),
        ("point_lights", TriPointLight * TRI_MAX_POINT_LIGHTS),
    ]


class TriMaterialRecord(C.Structure):
    _fields_ = [("base_color_factor", C.c_float * 4), ("material_factors", C.c_float * 4)]


class TriConfig(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("band_y0", C.c_uint32),
        ("band_y1", C.c_uint32),
        ("device", C.c_int32),
        ("flags", C.c_uint32),
    ]


class TriTiming(C.Structure):
    _fields_ = [
        ("frames", C.c_uint64),
        ("ms_vertex", C.c_double),
        ("ms_setup", C.c_double),
        ("ms_shadow", C.c_double),
        ("ms_raster", C.c_double),
        ("ms_frame", C.c_double),
        ("reserved", C.c_double),
    ]


class TriFrameStats(C.Structure):
    _fields_ = [
        ("triangles_in", C.c_uint64),
        ("triangles_setup", C.c_uint64),
        ("triangles_clipped", C.c_uint64),
        ("bin_entries", C.c_uint64),
        ("vertices_shaded", C.c_uint64),
        ("bins_x", C.c_uint32),
        ("bins_y", C.c_uint32),
        ("bin_size", C.c_uint32),
        ("path", C.c_uint32),
    ]


# tri_frame_stats.path bits (include/tri_raster.h)
TRI_PATH_ONE_DRAW, TRI_PATH_VARY_OBJ, TRI_PATH_OBJ_XFORM, TRI_PATH_OBJ_UCOL, TRI_PATH_SHADOW = 0x1, 0x2, 0x4, 0x8, 0x10
TRI_PATH_OBJ48 = 0x20
TRI_PATH_IDX_ROUTE = 0x40
TRI_PATH_EXACT = 0x80
# a frame-kind instantiation shaded the frame; its TRI_KIND_* switches at (path >> TRI_PATH_KIND_SHIFT) & TRI_KIND_MASK
TRI_PATH_KIND, TRI_PATH_KIND_SHIFT = 0x100, 16
TRI_KIND_XFORM, TRI_KIND_UCOL, TRI_KIND_SUN, TRI_KIND_DEPTH, TRI_KIND_SKYQ, TRI_KIND_LIGHTS = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
TRI_KIND_MASK = 0x3F

# the delta bit-plane band format (include/tri_raster.h)
TRI_DBP_SLOT_PIXELS, TRI_DBP_MIN_SLOT, TRI_DBP_MAX_SLOT, TRI_DBP_MAX_BANDS = 4096, 176, 12448, 16


class TriShadowConfig(C.Structure):
    _fields_ = [
        ("size", C.c_uint32),
        ("flags", C.c_uint32),
        ("depth_bias", C.c_float),
        ("slope_bias", C.c_float),
        ("light_view_proj", C.c_float * 16),
    ]


def make_shadow(light_view_proj, size=2048, depth_bias=0.001, slope_bias=2.0):
    s = TriShadowConfig()
    s.size, s.flags, s.depth_bias, s.slope_bias = size, 0, depth_bias, slope_bias
    s.light_view_proj = mat_to_c(light_view_proj)
    return s


# tri_upload_skybox_ex
TRI_SKY_FMT_RGBA8_SRGB, TRI_SKY_FMT_RGBA8_UNORM, TRI_SKY_FMT_RGBA16F = 0, 1, 2
TRI_SKYBOX_PREFILL = 0x1


class TriSkyboxDesc(C.Structure):
    _fields_ = [("format", C.c_uint32), ("size", C.c_uint32), ("mip_count", C.c_uint32), ("flags", C.c_uint32),
                ("texels", C.c_void_p), ("bytes", C.c_uint64)]


TRI_FORMAT_B8G8R8A8_UNORM = 44


class TriImage(C.Structure):
    _fields_ = [
        ("device_ptr", C.c_void_p),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("pitch_bytes", C.c_uint32),
        ("format", C.c_uint32),
        ("device", C.c_int32),
        ("reserved", C.c_uint32),
    ]


# entity ids (include/tri_raster.h): the id image's format, one picked pixel, the selection outline
TRI_FORMAT_R32_UINT = 98
TRI_MAX_OUTLINE_WIDTH = 8


class TriPickResult(C.Structure):
    _fields_ = [("id", C.c_uint32), ("depth_bits", C.c_uint32), ("has_depth", C.c_uint32), ("reserved", C.c_uint32)]


class TriOutline(C.Structure):
    _fields_ = [("draws", C.POINTER(C.c_uint32)), ("draw_count", C.c_uint32), ("rgba", C.c_float * 4),
                ("width_px", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(TriPickResult) == 16 and C.sizeof(TriOutline) == 40


# motion vectors (include/tri_raster.h): the motion image's format, the previous frame's camera and models
TRI_FORMAT_R32G32_SFLOAT = 103


class TriMotionHistory(C.Structure):
    _fields_ = [("prev_view", C.c_float * 16), ("prev_projection", C.c_float * 16), ("prev_models", C.POINTER(C.c_float)),
                ("draw_count", C.c_uint32), ("reserved", C.c_uint32)]


assert C.sizeof(TriMotionHistory) == 144


# history reprojection (include/tri_raster.h): the mask image's format, the mask bits, the pass's parameters
TRI_FORMAT_R8_UINT = 13
TRI_REPROJECT_NO_HISTORY, TRI_REPROJECT_NO_PROJ, TRI_REPROJECT_OUTSIDE, TRI_REPROJECT_ID, TRI_REPROJECT_DEPTH = 1, 2, 4, 8, 16
TRI_HISTORY_REDO = 1


TRI_RECORD_YUV444 = 0
TRI_RECORD_JPEG420 = 1


class TriRecordParams(C.Structure):
    _fields_ = [("format", C.c_uint32), ("quality", C.c_uint32), ("restart_mcus", C.c_uint32), ("flags", C.c_uint32)]


assert C.sizeof(TriRecordParams) == 16


class TriReprojectParams(C.Structure):
    _fields_ = [("depth_tolerance", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(TriReprojectParams) == 16


# temporal anti-aliasing (include/tri_raster.h): the accumulated colour's format, the mask bits, the flags, the parameters
TRI_FORMAT_R16G16B16A16_UNORM = 91
TRI_TAA_NO_HISTORY, TRI_TAA_NO_PROJ, TRI_TAA_OUTSIDE, TRI_TAA_ID, TRI_TAA_CLAMPED = 1, 2, 4, 8, 32
TRI_TAA_REDO, TRI_TAA_REJECT_ID = 1, 2


class TriTaaParams(C.Structure):
    _fields_ = [("alpha", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


assert C.sizeof(TriTaaParams) == 16


# temporal upscaling (include/tri_raster.h): the mask bits, the flags, the parameters
TRI_UPSCALE_NO_HISTORY, TRI_UPSCALE_NO_PROJ, TRI_UPSCALE_OUTSIDE, TRI_UPSCALE_ID = 1, 2, 4, 8
TRI_UPSCALE_CLAMPED, TRI_UPSCALE_NO_SAMPLE = 32, 64
TRI_UPSCALE_REDO, TRI_UPSCALE_REJECT_ID = 1, 2


class TriUpscaleParams(C.Structure):
    _fields_ = [("alpha", C.c_float), ("jitter", C.c_float * 2), ("flags", C.c_uint32)]


assert C.sizeof(TriUpscaleParams) == 16


class TriGroupConfig(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("device_count", C.c_uint32),
        ("display", C.c_uint32),
        ("devices", C.POINTER(C.c_int32)),
        ("flags", C.c_uint32),
        ("group_flags", C.c_uint32),
    ]


TRI_GROUP_NO_PACK = 0x1
TRI_GROUP_STAGE_BANDS = 0x2
TRI_GROUP_PACK_BGR24 = 0x4
TRI_XFER_ID_BYTES = 128
TRI_GRAB_HOST_COPY = 0x1  # tri_framegrab_create


# the frame generator (include/tri_raster.h)
TRI_NN_CONV3X3, TRI_NN_CONVT4X4 = 0, 1
TRI_NN_ACT_NONE, TRI_NN_ACT_RELU, TRI_NN_ACT_SIGMOID = 0, 1, 2
TRI_NN_MAX_CHANNELS = 1024
TRI_MAX_DIM = 8192


class TriNnConvDesc(C.Structure):
    _fields_ = [("op", C.c_uint32), ("stride", C.c_uint32), ("in_height", C.c_uint32), ("in_width", C.c_uint32),
                ("in_channels", C.c_uint32), ("out_channels", C.c_uint32), ("activation", C.c_uint32),
                ("reserved", C.c_uint32)]


assert C.sizeof(TriNnConvDesc) == 32


# text overlay (include/tri_raster.h; the scan chunk, per-round list capacity and bin edge of k_text_overlay are
# csrc/raster_launch.h's)
TRI_MAX_TEXT_QUADS = 65536
TRI_TEXT_SCAN_CHUNK, TRI_TEXT_LIST_CAP, TRI_TEXT_BIN = 64, 64, 32


class TriTextQuad(C.Structure):
    _fields_ = [("x0", C.c_float), ("y0", C.c_float), ("x1", C.c_float), ("y1", C.c_float),
                ("u0", C.c_float), ("v0", C.c_float), ("u1", C.c_float), ("v1", C.c_float),
                ("rgba", C.c_float * 4)]


# one row per quad: x0, y0, x1, y1, u0, v0, u1, v1, r, g, b, a
TEXT_QUAD_DTYPE = np.dtype(("<f4", 12))
assert C.sizeof(TriTextQuad) == 48 and TEXT_QUAD_DTYPE.itemsize == 48


# skeletal poses evaluated on the device (include/tri_raster.h)
TRI_POSE_MAX_BONES, TRI_POSE_PALETTE_BONES, TRI_POSE_BIND = 256, 128, 0xFFFFFFFF
TRI_POSE_MAX_INSTANCES, TRI_POSE_MAX_PALETTE = 65536, 1 << 24


class TriPoseBone(C.Structure):
    _fields_ = [("parent", C.c_int32), ("reserved", C.c_uint32 * 3), ("translation", C.c_float * 4),
                ("rotation", C.c_float * 4), ("scale", C.c_float * 4), ("inverse_bind", C.c_float * 16)]


class TriPoseChannel(C.Structure):
    _fields_ = [("bone", C.c_uint32), ("translation_first", C.c_uint32), ("translation_count", C.c_uint32),
                ("rotation_first", C.c_uint32), ("rotation_count", C.c_uint32), ("scale_first", C.c_uint32),
                ("scale_count", C.c_uint32), ("reserved", C.c_uint32)]


class TriPoseInstance(C.Structure):
    _fields_ = [("skeleton", C.c_uint32), ("clip", C.c_uint32), ("time", C.c_float), ("palette_offset", C.c_uint32)]


# the same records as numpy rows (rotation is w, x, y, z)
POSE_BONE_DTYPE = np.dtype([("parent", "<i4"), ("reserved", "<u4", 3), ("translation", "<f4", 4), ("rotation", "<f4", 4),
                            ("scale", "<f4", 4), ("inverse_bind", "<f4", 16)])
POSE_CHANNEL_DTYPE = np.dtype([("bone", "<u4"), ("translation_first", "<u4"), ("translation_count", "<u4"),
                               ("rotation_first", "<u4"), ("rotation_count", "<u4"), ("scale_first", "<u4"),
                               ("scale_count", "<u4"), ("reserved", "<u4")])
POSE_INSTANCE_DTYPE = np.dtype([("skeleton", "<u4"), ("clip", "<u4"), ("time", "<f4"), ("palette_offset", "<u4")])
assert C.sizeof(TriPoseBone) == POSE_BONE_DTYPE.itemsize == 128
assert C.sizeof(TriPoseChannel) == POSE_CHANNEL_DTYPE.itemsize == 32
assert C.sizeof(TriPoseInstance) == POSE_INSTANCE_DTYPE.itemsize == 16

# pose programs (tri_pose_graph)
TRI_POSE_STACK, TRI_POSE_MAX_OPS, TRI_POSE_NO_MASK = 8, 64, 0xFFFFFFFF
TRI_POSE_OP_REST, TRI_POSE_OP_CLIP, TRI_POSE_OP_BLEND, TRI_POSE_OP_ADD = 0, 1, 2, 3


class TriPoseOp(C.Structure):
    _fields_ = [("op", C.c_uint32), ("a", C.c_uint32), ("f", C.c_float), ("reserved", C.c_uint32)]


class TriPoseGraphInstance(C.Structure):
    _fields_ = [("skeleton", C.c_uint32), ("op_first", C.c_uint32), ("op_count", C.c_uint32),
                ("palette_offset", C.c_uint32)]


POSE_OP_DTYPE = np.dtype([("op", "<u4"), ("a", "<u4"), ("f", "<f4"), ("reserved", "<u4")])
POSE_GRAPH_INSTANCE_DTYPE = np.dtype([("skeleton", "<u4"), ("op_first", "<u4"), ("op_count", "<u4"),
                                      ("palette_offset", "<u4")])
assert C.sizeof(TriPoseOp) == POSE_OP_DTYPE.itemsize == 16
assert C.sizeof(TriPoseGraphInstance) == POSE_GRAPH_INSTANCE_DTYPE.itemsize == 16


class TriXferConfig(C.Structure):
    _fields_ = [("width", C.c_uint32), ("band_y", C.POINTER(C.c_uint32)), ("display", C.c_uint32),
                ("format", C.c_uint32), ("slot_bytes", C.c_uint32), ("alpha", C.c_uint32), ("nbuf", C.c_uint32)]
TRI_GROUP_FMT_BGRA32, TRI_GROUP_FMT_BGR24, TRI_GROUP_FMT_DBP = 0, 1, 2

for _s, _n in ((TriImage, 32), (TriGroupConfig, 32), (TriVertex, 100), (TriPushConstant, 128), (TriDraw, 144), (TriGlobalUbo, 480), (TriMaterialRecord, 32),
               (TriShadowConfig, 80)):
    assert C.sizeof(_s) == _n, (_s, C.sizeof(_s))

# every entry point include/tri_raster.h declares: (name, restype, argtypes)
CABI_FUNCTIONS = [
    ("tri_create", C.c_int, [C.POINTER(TriConfig), C.POINTER(C.c_void_p)]),
    ("tri_destroy", C.c_int, [C.c_void_p]),
    ("tri_set_stream", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_last_error", C.c_char_p, []),
    ("tri_abi_version", C.c_int, []),
    ("tri_upload_geometry", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]),
    ("tri_upload_materials", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_upload_texture", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("tri_upload_bone_palette", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_upload_skybox", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_upload_skybox_ex", C.c_int, [C.c_void_p, C.POINTER(TriSkyboxDesc)]),
    ("tri_upload_ai_frame", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("tri_set_frame", C.c_int, [C.c_void_p, C.POINTER(TriGlobalUbo), C.POINTER(C.c_float * 4)]),
    ("tri_set_draws", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_bind_output", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("tri_render", C.c_int, [C.c_void_p]),
    ("tri_synchronize", C.c_int, [C.c_void_p]),
    ("tri_readback", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("tri_blit_linear", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("tri_read_present", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_frame_alpha", C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    ("tri_pack_bgr24", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("tri_unpack_bgr24", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    ("tri_dbp_pack", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("tri_dbp_unpack", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("tri_dbp_bytes", C.c_uint64, [C.c_uint64, C.c_uint32]),
    ("tri_xfer_unique_id", C.c_int, [C.c_void_p]),
    ("tri_xfer_comm_create", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]),
    ("tri_xfer_comm_destroy", C.c_int, [C.c_void_p]),
    ("tri_xfer_create", C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]),
    ("tri_xfer_destroy", C.c_int, [C.c_void_p]),
    ("tri_xfer_bind_slot", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    ("tri_xfer_frame", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_uint32, C.c_uint32]),
    ("tri_xfer_synchronize", C.c_int, [C.c_void_p]),
    ("tri_xfer_wait", C.c_int, [C.c_void_p]),
    ("tri_xfer_set_timeout", C.c_int, [C.c_void_p, C.c_uint32]),
    ("tri_xfer_comm_count", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    ("tri_xfer_info", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    ("tri_xfer_loopback_create", C.c_int, [C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_xfer_loopback_destroy", C.c_int, [C.c_void_p]),
    ("tri_xfer_comm_create_loopback", C.c_int, [C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_void_p)]),
    ("tri_dbp_unpack_bands", C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.c_void_p]),
    ("tri_convert_yuv444", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("tri_recorder_create", C.c_int, [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_recorder_destroy", C.c_int, [C.c_void_p]),
    ("tri_recorder_capture", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    ("tri_recorder_wait", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_recorder_release", C.c_int, [C.c_void_p, C.c_uint32]),
    ("tri_recorder_create_ex", C.c_int, [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(TriRecordParams),
                                         C.POINTER(C.c_void_p)]),
    ("tri_recorder_capture_image", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    ("tri_recorder_wait_ex", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    ("tri_jpeg_header", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(TriRecordParams), C.c_void_p, C.c_uint32,
                                  C.POINTER(C.c_uint32)]),
    ("tri_jpeg_max_bytes", C.c_uint64, [C.c_uint32, C.c_uint32, C.POINTER(TriRecordParams)]),
    ("tri_convert_rgba_f32", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("tri_framegrab_create", C.c_int, [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_framegrab_destroy", C.c_int, [C.c_void_p]),
    ("tri_framegrab_capture", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    ("tri_framegrab_wait", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    ("tri_framegrab_release", C.c_int, [C.c_void_p, C.c_uint32]),
    ("tri_nn_pack_weights", C.c_int, [C.POINTER(TriNnConvDesc), C.c_void_p, C.c_void_p]),
    ("tri_nn_conv", C.c_int, [C.POINTER(TriNnConvDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p]),
    ("tri_framegen_create", C.c_int, [C.c_int32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_framegen_destroy", C.c_int, [C.c_void_p]),
    ("tri_framegen_info", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("tri_framegen_submit", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("tri_framegen_poll", C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    ("tri_framegen_wait", C.c_int, [C.c_void_p]),
    ("tri_framegen_output", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    ("tri_framegen_read_output", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_framegen_last_ms", C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    ("tri_upload_ai_frame_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    ("tri_read_ai_frame", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_get_stream", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    ("tri_font_create", C.c_int, [C.c_int32, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_font_destroy", C.c_int, [C.c_void_p]),
    ("tri_set_text", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_group_set_text", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32]),
    ("tri_animset_create", C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    ("tri_animset_destroy", C.c_int, [C.c_void_p]),
    ("tri_animset_add_skeleton", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_uint32)]),
    ("tri_animset_add_clip", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_uint32, C.c_float, C.POINTER(C.c_uint32)]),
    ("tri_pose_palette", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_read_bone_palette", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_group_pose_palette", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32]),
    ("tri_animset_add_mask", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    ("tri_pose_graph", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    ("tri_group_pose_graph", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_uint32]),
    ("tri_set_timing", C.c_int, [C.c_void_p, C.c_int]),
    ("tri_get_timing", C.c_int, [C.c_void_p, C.POINTER(TriTiming)]),
    ("tri_get_frame_stats", C.c_int, [C.c_void_p, C.POINTER(TriFrameStats)]),
    ("tri_set_shadow", C.c_int, [C.c_void_p, C.POINTER(TriShadowConfig)]),
    ("tri_shadow_fit_ortho", C.c_int, [C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3), C.POINTER(C.c_float * 3),
                                       C.POINTER(C.c_float * 16)]),
    ("tri_read_shadow_map", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_get_output", C.c_int, [C.c_void_p, C.POINTER(TriImage)]),
    ("tri_geometry_create", C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    ("tri_geometry_upload", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]),
    ("tri_geometry_destroy", C.c_int, [C.c_void_p]),
    ("tri_bind_geometry", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_group_create", C.c_int, [C.POINTER(TriGroupConfig), C.POINTER(C.c_void_p)]),
    ("tri_group_destroy", C.c_int, [C.c_void_p]),
    ("tri_group_context", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_group_upload_geometry", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]),
    ("tri_group_upload_materials", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_group_upload_texture", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("tri_group_upload_bone_palette", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_group_upload_skybox", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_group_upload_skybox_ex", C.c_int, [C.c_void_p, C.POINTER(TriSkyboxDesc)]),
    ("tri_group_upload_ai_frame", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("tri_group_set_shadow", C.c_int, [C.c_void_p, C.POINTER(TriShadowConfig)]),
    ("tri_group_set_frame", C.c_int, [C.c_void_p, C.POINTER(TriGlobalUbo), C.POINTER(C.c_float * 4)]),
    ("tri_group_set_draws", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    ("tri_group_render", C.c_int, [C.c_void_p]),
    ("tri_group_synchronize", C.c_int, [C.c_void_p]),
    ("tri_group_readback", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("tri_group_frame", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    ("tri_group_get_output", C.c_int, [C.c_void_p, C.POINTER(TriImage)]),
    ("tri_group_present", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_group_bind_geometry", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_group_blit_linear", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("tri_group_read_present", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_group_transfer_info", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("tri_group_transfer_format", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("tri_set_id_output", C.c_int, [C.c_void_p, C.c_int]),
    ("tri_read_ids", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_get_id_output", C.c_int, [C.c_void_p, C.POINTER(TriImage)]),
    ("tri_pick", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(TriPickResult)]),
    ("tri_pick_rect", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32,
                                C.POINTER(C.c_uint32)]),
    ("tri_set_outline", C.c_int, [C.c_void_p, C.POINTER(TriOutline)]),
    ("tri_get_id_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("tri_group_set_id_output", C.c_int, [C.c_void_p, C.c_int]),
    ("tri_group_read_ids", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_group_pick", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(TriPickResult)]),
    ("tri_set_motion_output", C.c_int, [C.c_void_p, C.c_int]),
    ("tri_set_motion_history", C.c_int, [C.c_void_p, C.POINTER(TriMotionHistory)]),
    ("tri_read_motion", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_get_motion_output", C.c_int, [C.c_void_p, C.POINTER(TriImage)]),
    ("tri_get_motion_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("tri_motion_matrices", C.c_int, [C.POINTER(TriGlobalUbo), C.POINTER(TriDraw), C.c_uint32, C.POINTER(TriMotionHistory),
                                      C.c_void_p]),
    ("tri_history_create", C.c_int, [C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_history_destroy", C.c_int, [C.c_void_p]),
    ("tri_history_reproject", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(TriReprojectParams)]),
    ("tri_history_reset", C.c_int, [C.c_void_p]),
    ("tri_history_read", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("tri_history_get_output", C.c_int, [C.c_void_p, C.POINTER(TriImage), C.POINTER(TriImage)]),
    ("tri_history_get_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("tri_taa_jitter", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_float * 2)]),
    ("tri_taa_jitter_projection", C.c_int, [C.POINTER(C.c_float * 16), C.c_float, C.c_float, C.c_uint32, C.c_uint32,
                                            C.POINTER(C.c_float * 16)]),
    ("tri_taa_create", C.c_int, [C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_taa_destroy", C.c_int, [C.c_void_p]),
    ("tri_taa_resolve", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(TriTaaParams)]),
    ("tri_taa_reset", C.c_int, [C.c_void_p]),
    ("tri_taa_read", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("tri_taa_get_output", C.c_int, [C.c_void_p, C.POINTER(TriImage), C.POINTER(TriImage), C.POINTER(TriImage)]),
    ("tri_taa_get_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("tri_taa_blit_linear", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("tri_upscale_create", C.c_int, [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    ("tri_upscale_destroy", C.c_int, [C.c_void_p]),
    ("tri_upscale_resolve", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(TriUpscaleParams)]),
    ("tri_upscale_reset", C.c_int, [C.c_void_p]),
    ("tri_upscale_read", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("tri_upscale_read_ids", C.c_int, [C.c_void_p, C.c_void_p]),
    ("tri_upscale_get_output", C.c_int, [C.c_void_p, C.POINTER(TriImage), C.POINTER(TriImage), C.POINTER(TriImage)]),
    ("tri_upscale_get_timing", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    ("tri_upscale_blit_linear", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    ("tri_upscale_jitter_period", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
]


def mat_to_c(m):
    """Column-major 4x4 (numpy [col][row] or flat 16) -> c_float*16."""
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(16))
    return (C.c_float * 16)(*a.tolist())


def make_draw(mesh_index, model, texture_slot=0, material_index=-1, tint=(1, 1, 1, 1), bone_offset=0, bone_count=0,
              texture_scale=(1, 1), texture_offset=(0, 0), tiling=1.0):
    """One MeshDrawCommand -> push constant, as RecordCommandBuffer fills it (Renderer.cpp:5129-5146)."""
    d = TriDraw()
    d.mesh_index = mesh_index
    pc = d.pc
    pc.model = mat_to_c(model)
    pc.tint = (C.c_float * 4)(*tint)
    pc.texture_scale = (C.c_float * 2)(*texture_scale)
    pc.texture_offset = (C.c_float * 2)(*texture_offset)
    pc.tiling_factor = tiling
    pc.texture_slot = texture_slot
    pc.use_material_override = 0
    pc.sort_bias = 0.0
    pc.material_index = material_index
    pc.bone_offset = bone_offset
    pc.bone_count = bone_count
    return d


def draws_array(draws):
    arr = (TriDraw * max(len(draws), 1))()
    for i, d in enumerate(draws):
        arr[i] = d
    return arr, len(draws)
