"""Python binding of the product C-ABI (libtri_raster.so, include/tri_raster.h).

This is plumbing for tests and bench.py: every call goes straight to the HIP library. There is no
CPU fallback — if the in-tree library is missing, import fails loudly.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.normpath(os.path.join(_HERE, "..", ".."))
LIB_PATH = os.path.join(PKG_ROOT, "lib", "libtri_raster.so")

_lib = None


class TriError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"tri_raster error {code}: {msg}")
        self.code = code


def load_library(path=None):
    """Load the HIP rasterizer library (built by `make -C 3d-renderer_amd`). TRI_RASTER_LIB may name
    another in-tree build of the same library (kernel-variant experiments)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("TRI_RASTER_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(f"HIP rasterizer library not built: {path} (run __graft_entry__.build())")
    lib = C.CDLL(path)
    variant = os.path.abspath(path) != os.path.abspath(LIB_PATH)
    for name, res, args in abi.CABI_FUNCTIONS:
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if not variant:  # the product library exports every entry point include/tri_raster.h declares
                raise
            continue  # an older A/B variant: entry points added since are absent there
        fn.restype = res
        fn.argtypes = args
    if lib.tri_abi_version() != abi.TRI_RASTER_ABI_VERSION:
        raise ImportError(f"tri_raster ABI version {lib.tri_abi_version()}, binding expects {abi.TRI_RASTER_ABI_VERSION}")
    _lib = lib
    return lib


def _check(rc):
    if rc != abi.TRI_OK:
        msg = _lib.tri_last_error().decode(errors="replace")
        raise TriError(rc, msg)


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _skybox_desc(texels, fmt, size, mip_count, flags):
    """(abi.TriSkyboxDesc, the array it points into): no conversion of the texels, only their bytes."""
    t = None if texels is None else np.ascontiguousarray(texels)
    d = abi.TriSkyboxDesc(int(fmt), int(size), int(mip_count), int(flags), t.ctypes.data if t is not None and t.size else None,
                          t.nbytes if t is not None else 0)
    return d, t


def shadow_fit_ortho(light_dir, aabb_min, aabb_max):
    """tri_shadow_fit_ortho (host-only): column-major light ortho * light view, as numpy [col][row]."""
    lib = load_library()
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])  # noqa: E731
    out = (C.c_float * 16)()
    _check(lib.tri_shadow_fit_ortho(C.byref(f3(light_dir)), C.byref(f3(aabb_min)), C.byref(f3(aabb_max)),
                                    C.byref(out)))
    return np.array(out[:], np.float32).reshape(4, 4)


class TriRaster:
    """One tri_ctx: a W x H framebuffer (optionally a row band) on one HIP device."""

    def __init__(self, width, height, band=None, device=-1, flags=0):
        lib = load_library()
        cfg = abi.TriConfig()
        cfg.width, cfg.height = width, height
        cfg.band_y0, cfg.band_y1 = band if band is not None else (0, 0)
        cfg.device = device
        cfg.flags = flags
        ctx = C.c_void_p()
        _check(lib.tri_create(C.byref(cfg), C.byref(ctx)))
        self._ctx = ctx
        self.width, self.height = width, height
        self.band = band if band is not None else (0, height)
        self.rows = self.band[1] - self.band[0]

    def close(self):
        if self._ctx:
            _lib.tri_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- uploads ----
    def upload_geometry(self, vertices, indices, meshes):
        v = np.ascontiguousarray(vertices, dtype=abi.VERTEX_DTYPE)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        m = np.ascontiguousarray(meshes, dtype=abi.MESH_RANGE_DTYPE)
        _check(_lib.tri_upload_geometry(self._ctx, _ptr(v), v.size, _ptr(i), i.size, _ptr(m), m.size))

    def upload_materials(self, records):
        n = len(records)
        arr = (abi.TriMaterialRecord * max(n, 1))()
        for k, (base, factors) in enumerate(records):
            arr[k].base_color_factor = (C.c_float * 4)(*base)
            arr[k].material_factors = (C.c_float * 4)(*factors)
        _check(_lib.tri_upload_materials(self._ctx, arr, n))

    def upload_texture(self, slot, rgba8):
        t = np.ascontiguousarray(rgba8, dtype=np.uint8)
        assert t.ndim == 3 and t.shape[2] == 4
        _check(_lib.tri_upload_texture(self._ctx, slot, _ptr(t), t.shape[1], t.shape[0]))

    def upload_bone_palette(self, mats):
        m = np.ascontiguousarray(mats, dtype=np.float32).reshape(-1, 16)
        _check(_lib.tri_upload_bone_palette(self._ctx, _ptr(m), m.shape[0]))

    def pose_palette(self, animset, instances):
        """tri_pose_palette: instances = rows of (skeleton, clip or abi.TRI_POSE_BIND, time, palette_offset), or a
        POSE_INSTANCE_DTYPE array; empty drops the posed suffix."""
        p = _pose_instances(instances)
        _check(_lib.tri_pose_palette(self._ctx, animset._s if animset is not None else None, _ptr(p) if p.size else None,
                                     p.size))

    def pose_graph(self, animset, instances, ops):
        """tri_pose_graph: instances = rows of (skeleton, op_first, op_count, palette_offset), ops = rows of
        (op, a, f) (or the POSE_GRAPH_INSTANCE_DTYPE / POSE_OP_DTYPE arrays); no instances drops the posed suffix."""
        p, o = _pose_graph_records(instances, ops)
        _check(_lib.tri_pose_graph(self._ctx, animset._s if animset is not None else None, _ptr(p) if p.size else None,
                                   p.size, _ptr(o) if o.size else None, o.size))

    def read_bone_palette(self, count):
        """tri_read_bone_palette: float32 [count, 16], column-major matrices."""
        out = np.empty((count, 16), dtype=np.float32)
        _check(_lib.tri_read_bone_palette(self._ctx, _ptr(out) if count else None, count))
        return out

    def upload_ai_frame(self, rgba):
        """rgba: uint8 [h, w, 4] R8G8B8A8_UNORM AI frame (Default.frag's blend), or None to remove it."""
        if rgba is None:
            _check(_lib.tri_upload_ai_frame(self._ctx, None, 0, 0))
            return
        f = np.ascontiguousarray(rgba, dtype=np.uint8)
        if f.ndim != 3 or f.shape[2] != 4:
            raise ValueError("AI frame must be uint8 [h, w, 4]")
        _check(_lib.tri_upload_ai_frame(self._ctx, _ptr(f), f.shape[1], f.shape[0]))

    def upload_ai_frame_device(self, tensor_ptr, width, height, channels, behind=None):
        """tri_upload_ai_frame_device: pack a [height, width, channels] float32 tensor on this context's device into the
        blend frame, on the context's stream (`behind`: a FrameGenerator whose last job the stream waits for)."""
        _check(_lib.tri_upload_ai_frame_device(self._ctx, C.c_void_p(tensor_ptr) if tensor_ptr else None, width, height,
                                               channels, behind._g if behind is not None else None))

    def read_ai_frame(self, width, height):
        """The blend frame as uint8 [height, width, 4] (R, G, B, A), after the context's stream has drained."""
        out = np.empty((height, width, 4), dtype=np.uint8)
        _check(_lib.tri_read_ai_frame(self._ctx, _ptr(out)))
        return out

    def upload_skybox(self, faces):
        """faces: uint8 [6, n, n, 4] sRGB (+X,-X,+Y,-Y,+Z,-Z), or None to remove the skybox."""
        if faces is None:
            _check(_lib.tri_upload_skybox(self._ctx, None, 0))
            return
        f = np.ascontiguousarray(faces, dtype=np.uint8)
        if f.ndim != 4 or f.shape[0] != 6 or f.shape[1] != f.shape[2] or f.shape[3] != 4:
            raise ValueError("skybox faces must be uint8 [6, n, n, 4]")
        _check(_lib.tri_upload_skybox(self._ctx, _ptr(f), f.shape[1]))

    def upload_skybox_ex(self, texels, fmt, size, mip_count=1, flags=0):
        """tri_upload_skybox_ex: `texels` is the whole chain as one contiguous array (level-major, then face, then rows;
        uint8 RGBA for the 8-bit formats, float16 or uint16 RGBA for abi.TRI_SKY_FMT_RGBA16F), or None to remove the
        skybox."""
        desc, keep = _skybox_desc(texels, fmt, size, mip_count, flags)  # (keep: the bytes the descriptor points at)
        _check(_lib.tri_upload_skybox_ex(self._ctx, C.byref(desc)))
        del keep

    def set_shadow(self, cfg):
        """tri_set_shadow: an abi.TriShadowConfig, or None to switch the shadow pre-pass off."""
        _check(_lib.tri_set_shadow(self._ctx, C.byref(cfg) if cfg is not None else None))
        self._shadow_size = int(cfg.size) if cfg is not None else 0

    def read_shadow_map(self):
        out = np.empty((self._shadow_size, self._shadow_size), np.uint32)
        _check(_lib.tri_read_shadow_map(self._ctx, _ptr(out)))
        return out

    # ---- frame ----
    def set_frame(self, ubo, clear=(0.005, 0.005, 0.005, 1.0)):
        cl = (C.c_float * 4)(*clear)
        _check(_lib.tri_set_frame(self._ctx, C.byref(ubo), C.byref(cl)))

    def set_draws(self, draws):
        arr, n = abi.draws_array(draws)
        _check(_lib.tri_set_draws(self._ctx, arr, n))

    def set_text(self, font, quads):
        """tri_set_text: float32 [n, 12] rows (x0, y0, x1, y1, u0, v0, u1, v1, r, g, b, a) composited over every
        following frame in row order; font None or no rows removes the overlay."""
        q = _text_quads(quads)
        _check(_lib.tri_set_text(self._ctx, font._f if font is not None else None, _ptr(q), q.shape[0]))

    def set_stream(self, stream_ptr):
        _check(_lib.tri_set_stream(self._ctx, C.c_void_p(stream_ptr) if stream_ptr else None))

    def frame_alpha(self):
        """tri_frame_alpha: the alpha byte every pixel of the next frame has, or -1 if not provably uniform."""
        a = C.c_int32()
        _check(_lib.tri_frame_alpha(self._ctx, C.byref(a)))
        return a.value

    def bind_geometry(self, geometry):
        """tri_bind_geometry: reference a shared TriGeometry (None: back to the context's own)."""
        _check(_lib.tri_bind_geometry(self._ctx, geometry._g if geometry is not None else None))

    def output_image(self):
        img = abi.TriImage()
        _check(_lib.tri_get_output(self._ctx, C.byref(img)))
        return img

    def bind_output(self, color_ptr, depth_ptr):
        _check(_lib.tri_bind_output(self._ctx, C.c_void_p(color_ptr) if color_ptr else None,
                                    C.c_void_p(depth_ptr) if depth_ptr else None))

    def render(self):
        _check(_lib.tri_render(self._ctx))

    def synchronize(self):
        _check(_lib.tri_synchronize(self._ctx))

    def readback(self, depth=True):
        """Returns (bgra uint8 [rows, W, 4], depth uint32 bits [rows, W] or None)."""
        col = np.empty((self.rows, self.width, 4), dtype=np.uint8)
        dep = np.empty((self.rows, self.width), dtype=np.uint32) if depth else None
        _check(_lib.tri_readback(self._ctx, _ptr(col), _ptr(dep) if depth else None))
        return col, dep

    def blit(self, width, height, dst_ptr=None):
        """tri_blit_linear: scale the frame to width x height (VK_FILTER_LINEAR presentation blit)."""
        _check(_lib.tri_blit_linear(self._ctx, C.c_void_p(dst_ptr) if dst_ptr else None, width, height))
        self._present = None if dst_ptr else (width, height)  # a caller-owned dst leaves the owned target stale

    def read_present(self):
        w, h = getattr(self, "_present", None) or (1, 1)  # nothing owned to read: the library reports TRI_E_STATE
        out = np.empty((h, w, 4), dtype=np.uint8)
        _check(_lib.tri_read_present(self._ctx, _ptr(out)))
        return out

    def render_frame(self, retries=2):
        """render + synchronize, re-rendering once after an internal-buffer overflow (buffers grow)."""
        for attempt in range(retries + 1):
            self.render()
            try:
                self.synchronize()
                return
            except TriError as e:
                if e.code != abi.TRI_E_OVERFLOW or attempt == retries:
                    raise

    # ---- entity ids ----
    def set_id_output(self, enable=True):
        """tri_set_id_output: every following render also writes the per-pixel draw ids."""
        _check(_lib.tri_set_id_output(self._ctx, 1 if enable else 0))

    def read_ids(self):
        """tri_read_ids: uint32 [rows, W]; 0 = background, else the draw's index in set_draws' list + 1."""
        out = np.empty((self.rows, self.width), dtype=np.uint32)
        _check(_lib.tri_read_ids(self._ctx, _ptr(out)))
        return out

    def id_image(self):
        img = abi.TriImage()
        _check(_lib.tri_get_id_output(self._ctx, C.byref(img)))
        return img

    def pick(self, x, y):
        """tri_pick: (id, depth bits or None under TRI_FLAG_NO_DEPTH_OUTPUT) of full-frame pixel (x, y)."""
        p = abi.TriPickResult()
        _check(_lib.tri_pick(self._ctx, int(x), int(y), C.byref(p)))
        return p.id, (p.depth_bits if p.has_depth else None)

    def pick_rect(self, x0, y0, x1, y1, draw_count):
        """tri_pick_rect: the sorted draw indices with a pixel inside the inclusive rectangle."""
        return _pick_rect(lambda *a: _lib.tri_pick_rect(self._ctx, *a), x0, y0, x1, y1, draw_count)

    def set_outline(self, draws, rgba=(1.0, 0.6, 0.0, 1.0), width_px=2):
        """tri_set_outline: outline the listed draws on every following frame; draws None removes the outline."""
        if draws is None:
            _check(_lib.tri_set_outline(self._ctx, None))
            return
        d = np.ascontiguousarray(draws, dtype=np.uint32).reshape(-1)
        o = abi.TriOutline()
        o.draws = d.ctypes.data_as(C.POINTER(C.c_uint32)) if d.size else None
        o.draw_count = d.size
        o.rgba = (C.c_float * 4)(*[float(c) for c in rgba])
        o.width_px = int(width_px)
        _check(_lib.tri_set_outline(self._ctx, C.byref(o)))

    def id_timing(self):
        """tri_get_id_timing: (summed ms of k_id_raster, timed frames that ran it)."""
        ms, n = C.c_double(), C.c_uint64()
        _check(_lib.tri_get_id_timing(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- motion vectors ----
    def set_motion_output(self, enable=True):
        """tri_set_motion_output: every following render also writes the per-pixel motion (needs the id output)."""
        _check(_lib.tri_set_motion_output(self._ctx, 1 if enable else 0))

    def set_motion_history(self, prev_view=None, prev_projection=None, prev_models=None, draw_count=None):
        """tri_set_motion_history: the previous frame's view and projection (16 floats each, column-major) and, per
        draw of the current list, its previous model ([n, 16] column-major; None: the current one). No view: no
        history. draw_count overrides the models' count (for the error cases)."""
        if prev_view is None:
            _check(_lib.tri_set_motion_history(self._ctx, None))
            return
        h, _keep = _motion_history(prev_view, prev_projection, prev_models, draw_count)
        _check(_lib.tri_set_motion_history(self._ctx, C.byref(h)))

    def read_motion(self):
        """tri_read_motion: float32 [rows, W, 2], (x, y) in pixels: where the pixel's surface lay one frame ago,
        minus the pixel."""
        out = np.empty((self.rows, self.width, 2), dtype=np.float32)
        _check(_lib.tri_read_motion(self._ctx, _ptr(out)))
        return out

    def motion_image(self):
        img = abi.TriImage()
        _check(_lib.tri_get_motion_output(self._ctx, C.byref(img)))
        return img

    def motion_timing(self):
        """tri_get_motion_timing: (summed ms of k_motion, timed frames that ran it)."""
        ms, n = C.c_double(), C.c_uint64()
        _check(_lib.tri_get_motion_timing(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def set_timing(self, enable, period=1):
        """Per-stage HIP-event timing of every `period`-th frame (enable=False: off)."""
        _check(_lib.tri_set_timing(self._ctx, int(period) if enable else 0))

    def timing(self):
        t = abi.TriTiming()
        _check(_lib.tri_get_timing(self._ctx, C.byref(t)))
        return {k: getattr(t, k) for k, _ in abi.TriTiming._fields_}

    def frame_stats(self):
        s = abi.TriFrameStats()
        _check(_lib.tri_get_frame_stats(self._ctx, C.byref(s)))
        return {k: getattr(s, k) for k, _ in abi.TriFrameStats._fields_}


def _motion_history(prev_view, prev_projection, prev_models, draw_count=None):
    """(abi.TriMotionHistory, the array it points into)."""
    h = abi.TriMotionHistory()
    h.prev_view = (C.c_float * 16)(*np.asarray(prev_view, np.float32).reshape(16).tolist())
    h.prev_projection = (C.c_float * 16)(*np.asarray(prev_projection, np.float32).reshape(16).tolist())
    m = None
    if prev_models is not None:
        m = np.ascontiguousarray(prev_models, dtype=np.float32).reshape(-1, 16)
        h.prev_models = m.ctypes.data_as(C.POINTER(C.c_float))
        h.draw_count = m.shape[0]
    if draw_count is not None:
        h.draw_count = int(draw_count)
    return h, m


def motion_matrices(ubo, draws, history=None):
    """tri_motion_matrices (host-only): the reprojection table of a frame, float32 [len(draws) + 1, 4, 4] with
    [k, i, j] = R_k[i][j]; row 0 is the background's. history: None, or (prev_view, prev_projection, prev_models or
    None[, draw_count]) as TriRaster.set_motion_history takes them."""
    lib = load_library()
    arr, n = abi.draws_array(draws)
    out = np.empty((n + 1, 4, 4), dtype=np.float32)
    h = keep = None
    if history is not None:
        h, keep = _motion_history(*history)
    _check(lib.tri_motion_matrices(C.byref(ubo), arr, n, C.byref(h) if h is not None else None, _ptr(out)))
    return out


class _TemporalObject:
    """What TriHistory, TriTaa and TriUpscale share: the handle's lifetime, reset and timing. A subclass names its
    destroy, reset and get_timing entry points and sets self._h."""

    _destroy = _reset = _timing = None

    def close(self):
        if self._h:
            getattr(_lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        _check(getattr(_lib, self._reset)(self._h))

    def timing(self):
        """get_timing: (summed ms of the stamped passes, their number)."""
        ms, n = C.c_double(), C.c_uint64()
        _check(getattr(_lib, self._timing)(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value


class TriHistory(_TemporalObject):
    """tri_history: the previous frame of one view (colour, ids, depth) outside any context, and the pass that warps it
    by a rendered frame's motion."""

    _destroy, _reset, _timing = "tri_history_destroy", "tri_history_reset", "tri_history_get_timing"

    def __init__(self, width, height, device=-1):
        lib = load_library()
        h = C.c_void_p()
        _check(lib.tri_history_create(device, width, height, C.byref(h)))
        self._h = h
        self.width, self.height = width, height

    def reproject(self, raster, depth_tolerance=0.0, redo=False, flags=None):
        """tri_history_reproject behind the raster's last render (asynchronous). flags overrides redo's bit (for the
        error cases)."""
        p = abi.TriReprojectParams(float(depth_tolerance), (abi.TRI_HISTORY_REDO if redo else 0) if flags is None else flags)
        _check(_lib.tri_history_reproject(self._h, raster._ctx, C.byref(p)))

    def read(self):
        """tri_history_read: (warped colour uint8 [H, W, 4] B G R A, mask uint8 [H, W])."""
        col = np.empty((self.height, self.width, 4), dtype=np.uint8)
        mask = np.empty((self.height, self.width), dtype=np.uint8)
        _check(_lib.tri_history_read(self._h, _ptr(col), _ptr(mask)))
        return col, mask

    def images(self):
        """tri_history_get_output: (colour, mask) as abi.TriImage."""
        col, mask = abi.TriImage(), abi.TriImage()
        _check(_lib.tri_history_get_output(self._h, C.byref(col), C.byref(mask)))
        return col, mask


def taa_jitter(index, period):
    """tri_taa_jitter (host-only): the sub-pixel offset of frame `index`, (x, y) in pixels as float32."""
    lib = load_library()
    xy = (C.c_float * 2)()
    _check(lib.tri_taa_jitter(index, period, C.byref(xy)))
    return np.float32(xy[0]), np.float32(xy[1])


def taa_jitter_projection(projection, jx, jy, width, height):
    """tri_taa_jitter_projection (host-only): the column-major projection (16 floats, any shape) with every projected
    point moved by (jx, jy) pixels; float32 [16]."""
    lib = load_library()
    src = (C.c_float * 16)(*np.asarray(projection, np.float32).reshape(16).tolist())
    out = (C.c_float * 16)()
    _check(lib.tri_taa_jitter_projection(C.byref(src), jx, jy, width, height, C.byref(out)))
    return np.array(out[:], dtype=np.float32)


class TriTaa(_TemporalObject):
    """tri_taa: the accumulated colour of one view (16-bit) outside any context, and the pass that resolves a jittered
    frame over it."""

    _destroy, _reset, _timing = "tri_taa_destroy", "tri_taa_reset", "tri_taa_get_timing"

    def __init__(self, width, height, device=-1):
        lib = load_library()
        h = C.c_void_p()
        _check(lib.tri_taa_create(device, width, height, C.byref(h)))
        self._h = h
        self.width, self.height = width, height

    def resolve(self, raster, alpha=0.1, reject_ids=True, redo=False, flags=None):
        """tri_taa_resolve behind the raster's last render (asynchronous). flags overrides the two switches' bits (for
        the error cases)."""
        bits = (abi.TRI_TAA_REDO if redo else 0) | (abi.TRI_TAA_REJECT_ID if reject_ids else 0)
        p = abi.TriTaaParams(float(alpha), bits if flags is None else flags)
        _check(_lib.tri_taa_resolve(self._h, raster._ctx, C.byref(p)))

    def read(self):
        """tri_taa_read: (resolved uint8 [H, W, 4] B G R A, accumulated uint16 [H, W, 4] B G R A, mask uint8 [H, W])."""
        col = np.empty((self.height, self.width, 4), dtype=np.uint8)
        acc = np.empty((self.height, self.width, 4), dtype=np.uint16)
        mask = np.empty((self.height, self.width), dtype=np.uint8)
        _check(_lib.tri_taa_read(self._h, _ptr(col), _ptr(acc), _ptr(mask)))
        return col, acc, mask

    def images(self):
        """tri_taa_get_output: (resolved, accumulated, mask) as abi.TriImage."""
        col, acc, mask = abi.TriImage(), abi.TriImage(), abi.TriImage()
        _check(_lib.tri_taa_get_output(self._h, C.byref(col), C.byref(acc), C.byref(mask)))
        return col, acc, mask

    def blit(self, raster, width, height, dst_ptr=None):
        """tri_taa_blit_linear: the resolved image scaled to width x height into dst_ptr, or into the raster's present
        image (TriRaster.read_present)."""
        _check(_lib.tri_taa_blit_linear(self._h, raster._ctx, C.c_void_p(dst_ptr) if dst_ptr else None, width, height))
        raster._present = None if dst_ptr else (width, height)


def upscale_jitter_period(render_w, render_h, out_w, out_h):
    """tri_upscale_jitter_period (host-only): eight samples per output pixel's area, at most 64."""
    lib = load_library()
    n = C.c_uint32()
    _check(lib.tri_upscale_jitter_period(render_w, render_h, out_w, out_h, C.byref(n)))
    return n.value


class TriUpscale(_TemporalObject):
    """tri_upscale: the accumulated colour of one view at an output extent (16-bit) outside any context, and the pass that
    resolves a jittered frame of the render extent over it."""

    _destroy, _reset, _timing = "tri_upscale_destroy", "tri_upscale_reset", "tri_upscale_get_timing"

    def __init__(self, render_w, render_h, out_w, out_h, device=-1):
        lib = load_library()
        h = C.c_void_p()
        _check(lib.tri_upscale_create(device, render_w, render_h, out_w, out_h, C.byref(h)))
        self._h = h
        self.render_width, self.render_height = render_w, render_h
        self.width, self.height = out_w, out_h

    def resolve(self, raster, jitter=(0.0, 0.0), alpha=0.1, reject_ids=True, redo=False, flags=None):
        """tri_upscale_resolve behind the raster's last render (asynchronous). jitter: the one the frame was rendered
        under, in render pixels. flags overrides the two switches' bits (for the error cases)."""
        bits = (abi.TRI_UPSCALE_REDO if redo else 0) | (abi.TRI_UPSCALE_REJECT_ID if reject_ids else 0)
        p = abi.TriUpscaleParams(float(alpha), (C.c_float * 2)(float(jitter[0]), float(jitter[1])), bits if flags is None else flags)
        _check(_lib.tri_upscale_resolve(self._h, raster._ctx, C.byref(p)))

    def read(self):
        """tri_upscale_read: (resolved uint8 [Ho, Wo, 4] B G R A, accumulated uint16 [Ho, Wo, 4], mask uint8 [Ho, Wo])."""
        col = np.empty((self.height, self.width, 4), dtype=np.uint8)
        acc = np.empty((self.height, self.width, 4), dtype=np.uint16)
        mask = np.empty((self.height, self.width), dtype=np.uint8)
        _check(_lib.tri_upscale_read(self._h, _ptr(col), _ptr(acc), _ptr(mask)))
        return col, acc, mask

    def read_ids(self):
        """tri_upscale_read_ids: the ids the last pass stored, uint32 [Hr, Wr]."""
        ids = np.empty((self.render_height, self.render_width), dtype=np.uint32)
        _check(_lib.tri_upscale_read_ids(self._h, _ptr(ids)))
        return ids

    def images(self):
        """tri_upscale_get_output: (resolved, accumulated, mask) as abi.TriImage."""
        col, acc, mask = abi.TriImage(), abi.TriImage(), abi.TriImage()
        _check(_lib.tri_upscale_get_output(self._h, C.byref(col), C.byref(acc), C.byref(mask)))
        return col, acc, mask

    def blit(self, raster, width, height, dst_ptr=None):
        """tri_upscale_blit_linear: the resolved image scaled to width x height into dst_ptr, or into the raster's
        present image (TriRaster.read_present)."""
        _check(_lib.tri_upscale_blit_linear(self._h, raster._ctx, C.c_void_p(dst_ptr) if dst_ptr else None, width, height))
        raster._present = None if dst_ptr else (width, height)


def _pick_rect(call, x0, y0, x1, y1, draw_count):
    words = max((int(draw_count) + 31) // 32, 1)
    bits = np.zeros(words, dtype=np.uint32)
    n = C.c_uint32()
    _check(call(int(x0), int(y0), int(x1), int(y1), _ptr(bits), words, C.byref(n)))
    found = [d for d in range(int(draw_count)) if (int(bits[d // 32]) >> (d % 32)) & 1]
    assert len(found) == n.value, (found, n.value)
    return found


def _text_quads(quads):
    q = np.ascontiguousarray(quads if quads is not None else np.zeros((0, 12)), dtype=np.float32)
    if q.size == 0:
        return q.reshape(0, 12)
    if q.ndim != 2 or q.shape[1] != 12:
        raise ValueError("text quads must be float32 [n, 12]")
    return q


class TriFont:
    """tri_font: one A8 coverage atlas (uint8 [h, w]) on one device."""

    def __init__(self, alpha, device=-1):
        lib = load_library()
        a = np.ascontiguousarray(alpha, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("a font atlas is uint8 [h, w]")
        f = C.c_void_p()
        _check(lib.tri_font_create(device, _ptr(a), a.shape[1], a.shape[0], C.byref(f)))
        self._f = f
        self.width, self.height = a.shape[1], a.shape[0]

    def close(self):
        if self._f:
            _lib.tri_font_destroy(self._f)
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _pose_instances(instances):
    if isinstance(instances, np.ndarray) and instances.dtype == abi.POSE_INSTANCE_DTYPE:
        return np.ascontiguousarray(instances)
    p = np.zeros(len(instances), dtype=abi.POSE_INSTANCE_DTYPE)
    for i, (skeleton, clip, time, offset) in enumerate(instances):
        p[i] = (skeleton, clip, time, offset)
    return p


def _pose_graph_records(instances, ops):
    if isinstance(instances, np.ndarray) and instances.dtype == abi.POSE_GRAPH_INSTANCE_DTYPE:
        p = np.ascontiguousarray(instances)
    else:
        p = np.zeros(len(instances), dtype=abi.POSE_GRAPH_INSTANCE_DTYPE)
        for i, (skeleton, first, count, offset) in enumerate(instances):
            p[i] = (skeleton, first, count, offset)
    if isinstance(ops, np.ndarray) and ops.dtype == abi.POSE_OP_DTYPE:
        o = np.ascontiguousarray(ops)
    else:
        o = np.zeros(len(ops), dtype=abi.POSE_OP_DTYPE)
        for i, (op, a, f) in enumerate(ops):
            o[i] = (op, a, f, 0)
    return p, o


class TriAnimSet:
    """tri_animset: skeletons, clips and masks on one device, posed by tri_pose_palette / tri_pose_graph."""

    def __init__(self, device=-1):
        lib = load_library()
        s = C.c_void_p()
        _check(lib.tri_animset_create(device, C.byref(s)))
        self._s = s

    def add_skeleton(self, bones, root_index=-1):
        """bones: POSE_BONE_DTYPE rows (decomposed defaults, rotation w, x, y, z); returns the skeleton index."""
        b = np.ascontiguousarray(bones, dtype=abi.POSE_BONE_DTYPE)
        out = C.c_uint32()
        _check(_lib.tri_animset_add_skeleton(self._s, _ptr(b), b.size, root_index, C.byref(out)))
        return out.value

    def add_clip(self, skeleton, channels, vec_times, vec_values, quat_times, quat_values, duration):
        """channels: POSE_CHANNEL_DTYPE rows; vec_values [n, 3]; quat_values [n, 4] (w, x, y, z); returns the clip index."""
        ch = np.ascontiguousarray(channels, dtype=abi.POSE_CHANNEL_DTYPE)
        vt = np.ascontiguousarray(vec_times, dtype=np.float32).reshape(-1)
        vv = np.ascontiguousarray(vec_values, dtype=np.float32).reshape(-1, 3)
        qt = np.ascontiguousarray(quat_times, dtype=np.float32).reshape(-1)
        qv = np.ascontiguousarray(quat_values, dtype=np.float32).reshape(-1, 4)
        assert vt.size == vv.shape[0] and qt.size == qv.shape[0]
        out = C.c_uint32()
        opt = lambda a: _ptr(a) if a.size else None  # noqa: E731
        _check(_lib.tri_animset_add_clip(self._s, skeleton, opt(ch), ch.size, opt(vt), opt(vv), vt.size, opt(qt), opt(qv),
                                         qt.size, duration, C.byref(out)))
        return out.value

    def add_mask(self, skeleton, weights):
        """tri_animset_add_mask: per-bone weights (shorter: the rest weigh 1.0; longer: dropped); returns the mask index."""
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        out = C.c_uint32()
        _check(_lib.tri_animset_add_mask(self._s, skeleton, _ptr(w) if w.size else None, w.size, C.byref(out)))
        return out.value

    def close(self):
        if self._s:
            _lib.tri_animset_destroy(self._s)
            self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class TriGeometry:
    """tri_geometry: meshes uploaded once on one device, bound by any number of contexts there."""

    def __init__(self, device=-1):
        lib = load_library()
        g = C.c_void_p()
        _check(lib.tri_geometry_create(device, C.byref(g)))
        self._g = g

    def upload(self, vertices, indices, meshes):
        v = np.ascontiguousarray(vertices, dtype=abi.VERTEX_DTYPE)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        m = np.ascontiguousarray(meshes, dtype=abi.MESH_RANGE_DTYPE)
        _check(_lib.tri_geometry_upload(self._g, _ptr(v), v.size, _ptr(i), i.size, _ptr(m), m.size))

    def close(self):
        if self._g:
            _lib.tri_geometry_destroy(self._g)
            self._g = None


def pack_bgr24(src_ptr, dst_ptr, pixels, alpha, flag_ptr=None, stream_ptr=None):
    """tri_pack_bgr24: B8G8R8A8 -> 3-byte BGR on the device, stream-ordered (flag: device uint32 set when an
    alpha byte differs from `alpha`)."""
    load_library()
    _check(_lib.tri_pack_bgr24(C.c_void_p(src_ptr), C.c_void_p(dst_ptr), pixels, alpha,
                               C.c_void_p(flag_ptr) if flag_ptr else None, C.c_void_p(stream_ptr) if stream_ptr else None))


def unpack_bgr24(src_ptr, dst_ptr, pixels, alpha, stream_ptr=None):
    """tri_unpack_bgr24: 3-byte BGR -> B8G8R8A8 with the given alpha, stream-ordered."""
    load_library()
    _check(_lib.tri_unpack_bgr24(C.c_void_p(src_ptr), C.c_void_p(dst_ptr), pixels, alpha,
                                 C.c_void_p(stream_ptr) if stream_ptr else None))


def dbp_pack(src_ptr, pixels, alpha, dst_ptr, slot_bytes, flags_ptr=None, stream_ptr=None):
    """tri_dbp_pack: B8G8R8A8 -> the delta bit-plane stream (slots of slot_bytes), stream-ordered; flags: device
    uint32[2] (bit 1 alpha mismatch, bit 2 slot overflow; the largest slot's bytes)."""
    load_library()
    _check(_lib.tri_dbp_pack(C.c_void_p(src_ptr), pixels, alpha, C.c_void_p(dst_ptr), slot_bytes,
                             C.c_void_p(flags_ptr) if flags_ptr else None, C.c_void_p(stream_ptr) if stream_ptr else None))


def dbp_unpack(src_ptr, pixels, alpha, slot_bytes, dst_ptr, stream_ptr=None):
    """tri_dbp_unpack: the delta bit-plane stream -> B8G8R8A8 with the given alpha, stream-ordered."""
    load_library()
    _check(_lib.tri_dbp_unpack(C.c_void_p(src_ptr), pixels, alpha, slot_bytes, C.c_void_p(dst_ptr),
                               C.c_void_p(stream_ptr) if stream_ptr else None))


def dbp_unpack_bands(src_ptrs, dst_ptrs, pixels, alpha, slot_bytes, stream_ptr=None):
    """tri_dbp_unpack_bands: several delta bit-plane streams (one slot size) -> their B8G8R8A8 bands, one launch."""
    load_library()
    k = len(src_ptrs)
    srcs = (C.c_void_p * max(k, 1))(*src_ptrs)
    dsts = (C.c_void_p * max(k, 1))(*dst_ptrs)
    npx = (C.c_uint64 * max(k, 1))(*pixels)
    _check(_lib.tri_dbp_unpack_bands(srcs, dsts, npx, k, alpha, slot_bytes, C.c_void_p(stream_ptr) if stream_ptr else None))


def dbp_bytes(pixels, slot_bytes):
    load_library()
    return int(_lib.tri_dbp_bytes(pixels, slot_bytes))


def convert_yuv444(src_ptr, width, height, pitch_bytes, dst_ptr, stream_ptr=None):
    """tri_convert_yuv444: B8G8R8A8 rows (pitch_bytes apart) -> the Y, U, V planes (3 * width * height bytes) on the
    device, stream-ordered."""
    load_library()
    _check(_lib.tri_convert_yuv444(C.c_void_p(src_ptr) if src_ptr else None, width, height, pitch_bytes,
                                   C.c_void_p(dst_ptr) if dst_ptr else None, C.c_void_p(stream_ptr) if stream_ptr else None))


def record_params(fmt=abi.TRI_RECORD_JPEG420, quality=90, restart_mcus=0, flags=0):
    return abi.TriRecordParams(fmt, quality, restart_mcus, flags)


def jpeg_header(width, height, quality=90, restart_mcus=0, capacity=1024, params=None):
    """tri_jpeg_header: the stream's bytes before the entropy-coded data (host only)."""
    load_library()
    p = params if params is not None else record_params(abi.TRI_RECORD_JPEG420, quality, restart_mcus)
    buf = (C.c_uint8 * max(capacity, 1))()
    n = C.c_uint32()
    _check(_lib.tri_jpeg_header(width, height, C.byref(p), buf, capacity, C.byref(n)))
    return bytes(buf[:n.value])


def jpeg_max_bytes(width, height, quality=90, restart_mcus=0, params=None):
    """tri_jpeg_max_bytes: the size no stream of this extent and these parameters exceeds (host only)."""
    load_library()
    p = params if params is not None else record_params(abi.TRI_RECORD_JPEG420, quality, restart_mcus)
    n = _lib.tri_jpeg_max_bytes(width, height, C.byref(p))
    if n == 0:
        _check(abi.TRI_E_INVALID)
    return n


class TriRecorder:
    """tri_recorder: `slots` device + pinned buffers of one extent; capture is asynchronous. fmt None is
    tri_recorder_create (YUV 4:4:4 planes); TRI_RECORD_YUV444 / TRI_RECORD_JPEG420 go through tri_recorder_create_ex."""

    def __init__(self, width, height, slots, device=-1, fmt=None, quality=90, restart_mcus=0, params=None):
        lib = load_library()
        r = C.c_void_p()
        if fmt is None and params is None:
            _check(lib.tri_recorder_create(device, width, height, slots, C.byref(r)))
        else:
            p = params if params is not None else record_params(fmt, quality, restart_mcus)
            _check(lib.tri_recorder_create_ex(device, width, height, slots, C.byref(p), C.byref(r)))
        self._r = r
        self.width, self.height, self.slots = width, height, slots

    def close(self):
        if self._r:
            _lib.tri_recorder_destroy(self._r)
            self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def capture(self, slot, raster):
        _check(_lib.tri_recorder_capture(self._r, slot, raster._ctx))

    def wait_pointer(self, slot):
        p = C.c_void_p()
        _check(_lib.tri_recorder_wait(self._r, slot, C.byref(p)))
        return p.value

    def wait(self, slot):
        """The slot's planes, uint8 [3, height, width]: a view of the pinned buffer, valid until release."""
        p = self.wait_pointer(slot)
        buf = (C.c_uint8 * (3 * self.width * self.height)).from_address(p)
        return np.frombuffer(buf, np.uint8).reshape(3, self.height, self.width)

    def capture_image(self, slot, src_ptr, pitch_bytes, stream_ptr=None):
        """tri_recorder_capture_image: the capture from any device image of the recorder's extent."""
        _check(_lib.tri_recorder_capture_image(self._r, slot, C.c_void_p(src_ptr) if src_ptr else None, pitch_bytes,
                                               C.c_void_p(stream_ptr) if stream_ptr else None))

    def wait_ex(self, slot):
        """The slot's product, uint8 [bytes]: a view of the pinned buffer, valid until release."""
        p, n = C.c_void_p(), C.c_uint64()
        _check(_lib.tri_recorder_wait_ex(self._r, slot, C.byref(p), C.byref(n)))
        return np.frombuffer((C.c_uint8 * n.value).from_address(p.value), np.uint8)

    def release(self, slot):
        _check(_lib.tri_recorder_release(self._r, slot))


def convert_rgba_f32(src_ptr, width, height, pitch_bytes, dst_ptr, stream_ptr=None):
    """tri_convert_rgba_f32: B8G8R8A8 rows (pitch_bytes apart) -> width * height * 4 float32 (R, G, B, A per pixel,
    byte * (1 / 255) in float32) on the device, stream-ordered."""
    load_library()
    _check(_lib.tri_convert_rgba_f32(C.c_void_p(src_ptr) if src_ptr else None, width, height, pitch_bytes,
                                     C.c_void_p(dst_ptr) if dst_ptr else None, C.c_void_p(stream_ptr) if stream_ptr else None))


class FrameGrab:
    """tri_framegrab: `slots` device float32 RGBA tensors of one extent (pinned host copies too with host_copy);
    capture is asynchronous."""

    def __init__(self, width, height, slots, device=-1, host_copy=False):
        lib = load_library()
        g = C.c_void_p()
        _check(lib.tri_framegrab_create(device, width, height, slots, abi.TRI_GRAB_HOST_COPY if host_copy else 0, C.byref(g)))
        self._g = g
        self.width, self.height, self.slots, self.host_copy = width, height, slots, host_copy

    def close(self):
        if self._g:
            _lib.tri_framegrab_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def capture(self, slot, raster):
        _check(_lib.tri_framegrab_capture(self._g, slot, raster._ctx))

    def wait_pointers(self, slot, host=True, device=True):
        """(pinned pointer or None, device pointer or None) of the slot, after the events they depend on."""
        h, d = C.c_void_p(), C.c_void_p()
        _check(_lib.tri_framegrab_wait(self._g, slot, C.byref(h) if host else None, C.byref(d) if device else None))
        return (h.value if host else None), (d.value if device else None)

    def wait(self, slot):
        """(the pinned tensor, float32 [height, width, 4], or None without host_copy; the device pointer). Both are
        valid until release."""
        h, d = self.wait_pointers(slot, host=self.host_copy)
        if h is None:
            return None, d
        buf = (C.c_float * (4 * self.width * self.height)).from_address(h)
        return np.frombuffer(buf, np.float32).reshape(self.height, self.width, 4), d

    def release(self, slot):
        _check(_lib.tri_framegrab_release(self._g, slot))


def copy_device_to_host(ptr, nbytes, device=0):
    """hipMemcpy of `nbytes` at a device pointer (a tri_image handle) into a numpy byte array."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipSetDevice.argtypes = [C.c_int]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = np.empty(nbytes, np.uint8)
    assert hip.hipSetDevice(device) == 0
    assert hip.hipMemcpy(out.ctypes.data, C.c_void_p(ptr), nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


def nn_pack_weights(desc, torch_weights):
    """tri_nn_pack_weights: torch's Conv2d / ConvTranspose2d weights (float32 array) in tri_nn_conv's layout."""
    load_library()
    src = np.ascontiguousarray(torch_weights, dtype=np.float32)
    out = np.empty(src.size, dtype=np.float32)
    _check(_lib.tri_nn_pack_weights(C.byref(desc), _ptr(src), _ptr(out)))
    return out


class FrameGenerator:
    """tri_framegen: the interpolation network for one frozen extent on one device, from a weights container (bytes).
    One job at a time, asynchronous on the generator's own stream."""

    def __init__(self, container, width, height, device=-1):
        lib = load_library()
        g = C.c_void_p()
        blob = bytes(container)
        _check(lib.tri_framegen_create(device, blob, len(blob), width, height, C.byref(g)))
        self._g = g
        self.width, self.height = width, height
        cin = C.c_uint32()
        _check(lib.tri_framegen_info(g, C.byref(cin), None, None))
        self.input_channels = cin.value

    def close(self):
        if self._g:
            _lib.tri_framegen_destroy(self._g)  # waits for a job in flight
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def submit(self, input_ptr, stream_ptr=None):
        """input_ptr: [height, width, input_channels] float32 on the device; copied on stream_ptr (None: the null stream)."""
        _check(_lib.tri_framegen_submit(self._g, C.c_void_p(input_ptr) if input_ptr else None,
                                        C.c_void_p(stream_ptr) if stream_ptr else None))

    def poll(self):
        """True once per job, when it has finished; never blocks."""
        done = C.c_int32()
        _check(_lib.tri_framegen_poll(self._g, C.byref(done)))
        return bool(done.value)

    def wait(self):
        _check(_lib.tri_framegen_wait(self._g))

    def output_pointer(self):
        p = C.c_void_p()
        _check(_lib.tri_framegen_output(self._g, C.byref(p)))
        return p.value

    def read_output(self):
        """The last finished job's output, float32 [height, width, 3]."""
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        _check(_lib.tri_framegen_read_output(self._g, _ptr(out)))
        return out

    def last_ms(self):
        ms = C.c_float()
        _check(_lib.tri_framegen_last_ms(self._g, C.byref(ms)))
        return ms.value


class TriGroup:
    """tri_group: one frame over N row-band contexts on the given devices (RCCL gather onto the display
    band's device; bands sharing that device render in place)."""

    def __init__(self, width, height, devices, display=0, flags=0, group_flags=0):
        lib = load_library()
        n = len(devices)
        self._devs = (C.c_int32 * n)(*devices)
        cfg = abi.TriGroupConfig(width, height, n, display, self._devs, flags, group_flags)
        g = C.c_void_p()
        _check(lib.tri_group_create(C.byref(cfg), C.byref(g)))
        self._g = g
        self.width, self.height, self.n = width, height, n

    def close(self):
        if self._g:
            _lib.tri_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def upload_geometry(self, vertices, indices, meshes):
        v = np.ascontiguousarray(vertices, dtype=abi.VERTEX_DTYPE)
        i = np.ascontiguousarray(indices, dtype=np.uint32)
        m = np.ascontiguousarray(meshes, dtype=abi.MESH_RANGE_DTYPE)
        _check(_lib.tri_group_upload_geometry(self._g, _ptr(v), v.size, _ptr(i), i.size, _ptr(m), m.size))

    def upload_materials(self, records):
        n = len(records)
        arr = (abi.TriMaterialRecord * max(n, 1))()
        for k, (base, factors) in enumerate(records):
            arr[k].base_color_factor = (C.c_float * 4)(*base)
            arr[k].material_factors = (C.c_float * 4)(*factors)
        _check(_lib.tri_group_upload_materials(self._g, arr, n))

    def upload_texture(self, slot, rgba8):
        t = np.ascontiguousarray(rgba8, dtype=np.uint8)
        _check(_lib.tri_group_upload_texture(self._g, slot, _ptr(t), t.shape[1], t.shape[0]))

    def upload_bone_palette(self, mats):
        m = np.ascontiguousarray(mats, dtype=np.float32).reshape(-1, 16)
        _check(_lib.tri_group_upload_bone_palette(self._g, _ptr(m), m.shape[0]))

    def upload_ai_frame(self, rgba):
        if rgba is None:
            _check(_lib.tri_group_upload_ai_frame(self._g, None, 0, 0))
            return
        f = np.ascontiguousarray(rgba, dtype=np.uint8)
        _check(_lib.tri_group_upload_ai_frame(self._g, _ptr(f), f.shape[1], f.shape[0]))

    def upload_skybox(self, faces):
        if faces is None:
            _check(_lib.tri_group_upload_skybox(self._g, None, 0))
            return
        f = np.ascontiguousarray(faces, dtype=np.uint8)
        _check(_lib.tri_group_upload_skybox(self._g, _ptr(f), f.shape[1]))

    def upload_skybox_ex(self, texels, fmt, size, mip_count=1, flags=0):
        desc, keep = _skybox_desc(texels, fmt, size, mip_count, flags)
        _check(_lib.tri_group_upload_skybox_ex(self._g, C.byref(desc)))
        del keep

    def set_shadow(self, cfg):
        _check(_lib.tri_group_set_shadow(self._g, C.byref(cfg) if cfg is not None else None))

    def set_frame(self, ubo, clear=(0.005, 0.005, 0.005, 1.0)):
        cl = (C.c_float * 4)(*clear)
        _check(_lib.tri_group_set_frame(self._g, C.byref(ubo), C.byref(cl)))

    def set_draws(self, draws):
        arr, n = abi.draws_array(draws)
        _check(_lib.tri_group_set_draws(self._g, arr, n))

    def set_text(self, fonts, quads):
        """tri_group_set_text: fonts = one TriFont per distinct device of the group (any order); None or no rows
        removes the overlay."""
        q = _text_quads(quads)
        if not fonts or q.shape[0] == 0:
            _check(_lib.tri_group_set_text(self._g, None, None, 0))
            return
        ndev = len(set(self._devs[:]))
        if len(fonts) < ndev:
            raise ValueError(f"{ndev} devices need {ndev} fonts")
        arr = (C.c_void_p * len(fonts))(*[f._f.value for f in fonts])
        _check(_lib.tri_group_set_text(self._g, arr, _ptr(q), q.shape[0]))

    def pose_graph(self, animsets, instances, ops):
        """tri_group_pose_graph: animsets = one TriAnimSet per distinct device of the group (any order)."""
        p, o = _pose_graph_records(instances, ops)
        if not p.size:
            _check(_lib.tri_group_pose_graph(self._g, None, None, 0, None, 0))
            return
        arr = (C.c_void_p * len(animsets))(*[s._s.value for s in animsets])
        _check(_lib.tri_group_pose_graph(self._g, arr, _ptr(p), p.size, _ptr(o) if o.size else None, o.size))

    def render(self):
        _check(_lib.tri_group_render(self._g))

    def synchronize(self):
        _check(_lib.tri_group_synchronize(self._g))

    def render_frame(self, retries=2):
        for attempt in range(retries + 1):
            self.render()
            try:
                self.synchronize()
                return
            except TriError as e:
                if e.code != abi.TRI_E_OVERFLOW or attempt == retries:
                    raise

    def readback(self, depth=True):
        col = np.empty((self.height, self.width, 4), dtype=np.uint8)
        dep = np.empty((self.height, self.width), dtype=np.uint32) if depth else None
        _check(_lib.tri_group_readback(self._g, _ptr(col), _ptr(dep) if depth else None))
        return col, dep

    def set_id_output(self, enable=True):
        _check(_lib.tri_group_set_id_output(self._g, 1 if enable else 0))

    def read_ids(self):
        """tri_group_read_ids: uint32 [H, W], every band's rows."""
        out = np.empty((self.height, self.width), dtype=np.uint32)
        _check(_lib.tri_group_read_ids(self._g, _ptr(out)))
        return out

    def pick(self, x, y):
        p = abi.TriPickResult()
        _check(_lib.tri_group_pick(self._g, int(x), int(y), C.byref(p)))
        return p.id, (p.depth_bits if p.has_depth else None)

    def frame_pointer(self):
        p, d = C.c_void_p(), C.c_int32()
        _check(_lib.tri_group_frame(self._g, C.byref(p), C.byref(d)))
        return p.value, d.value

    def output_image(self):
        img = abi.TriImage()
        _check(_lib.tri_group_get_output(self._g, C.byref(img)))
        return img

    def present(self, stream_ptr=None):
        """tri_group_present: the consumer fence on the most recent frame (after `stream_ptr`'s work, or now)."""
        _check(_lib.tri_group_present(self._g, C.c_void_p(stream_ptr) if stream_ptr else None))

    def bind_geometry(self, geometries):
        """tri_group_bind_geometry: caller-owned TriGeometry objects (one per device); [] = the group's own."""
        arr = (C.c_void_p * max(len(geometries), 1))(*[g._g.value for g in geometries])
        _check(_lib.tri_group_bind_geometry(self._g, len(geometries), arr))

    def context(self, band):
        """The band's tri_ctx handle (tri_group_context)."""
        c = C.c_void_p()
        _check(_lib.tri_group_context(self._g, band, C.byref(c)))
        return c

    def blit(self, width, height, dst_ptr=None):
        _check(_lib.tri_group_blit_linear(self._g, C.c_void_p(dst_ptr) if dst_ptr else None, width, height))
        self._present = None if dst_ptr else (width, height)

    def read_present(self):
        w, h = getattr(self, "_present", None) or (1, 1)  # nothing owned to read: the library reports TRI_E_STATE
        out = np.empty((h, w, 4), dtype=np.uint8)
        _check(_lib.tri_group_read_present(self._g, _ptr(out)))
        return out

    def transfer_info(self):
        """tri_group_transfer_info: (bytes per pixel on the links, inbound RCCL bytes) of the last frame."""
        bpp, inbound = C.c_uint32(), C.c_uint64()
        _check(_lib.tri_group_transfer_info(self._g, C.byref(bpp), C.byref(inbound)))
        return bpp.value, inbound.value

    def transfer_format(self):
        """tri_group_transfer_format: (TRI_GROUP_FMT_*, dbp slot bytes or 0) of the last frame."""
        fmt, slot = C.c_uint32(), C.c_uint32()
        _check(_lib.tri_group_transfer_format(self._g, C.byref(fmt), C.byref(slot)))
        return fmt.value, slot.value
