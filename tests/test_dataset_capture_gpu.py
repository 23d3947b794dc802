"""AI readback and dataset capture on the GPU: k_bgra_to_rgba_f32 (tri_convert_rgba_f32) against the numpy restatement
(tests/tensor_ref.py) with zero differing bits, the tri_framegrab slot protocol, and the shim's readback, dataset files
and AI output path end to end."""
import ctypes as C

import numpy as np
import pytest

import scene_cases as sc
import tensor_ref
import yuv_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _convert(src, width, height, pitch, dst):
    import torch
    from trident_raster import raster

    raster.convert_rgba_f32(src.data_ptr(), width, height, pitch, dst.data_ptr())  # the null stream, as torch's
    torch.cuda.synchronize()


def test_every_byte_value_in_every_channel():
    """64 x 16 = 1024 pixels = four runs of 256: each channel runs through all byte values in its own permutation."""
    import torch

    i = np.arange(1024, dtype=np.uint32)
    bgra = np.empty((16, 64, 4), np.uint8)
    flat = bgra.reshape(-1, 4)
    flat[:, 0] = i & 255                 # B: ascending
    flat[:, 1] = 255 - (i & 255)         # G: descending
    flat[:, 2] = (i * 7 + 3) & 255       # R: a stride coprime to 256
    flat[:, 3] = ((i & 255) ^ 0x5A)      # A: xor-scrambled
    for ch in range(4):
        assert set(flat[:256, ch].tolist()) == set(range(256))
    src = torch.from_numpy(bgra).to(DEV)
    dst = torch.zeros(1024 * 4, dtype=torch.float32, device=DEV)
    _convert(src, 64, 16, 64 * 4, dst)
    got = dst.cpu().numpy().reshape(16, 64, 4)
    want = tensor_ref.tensor_from_bgra(bgra)
    assert int((_bits(got) != _bits(want)).sum()) == 0
    assert got[flat.reshape(16, 64, 4)[..., [2, 1, 0, 3]] == 255].min() == np.float32(1.0)
    # a division by 255 instead of the multiply would differ on 126 byte values: the arithmetic is pinned
    div = tensor_ref.division_variant(bgra[..., [2, 1, 0, 3]])
    differing = np.unique(bgra[..., [2, 1, 0, 3]][_bits(got) != _bits(div)])
    assert len(differing) == 126


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("shape", [(1, 1), (3, 1), (5, 3), (63, 2), (64, 1), (65, 2), (257, 3)])
def test_ragged_shapes_and_guard_bytes(shape, offset):
    """Sizes around the wave and the 1024-item block; the output 16-B aligned (one 16-B store per pixel) and 4 bytes in
    (the dword path): exact, and nothing around it is written."""
    import torch

    w, h = shape
    rng = np.random.default_rng(1000 * w + 10 * h + offset)
    bgra = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    n, guard = 16 * w * h, 256
    src = torch.from_numpy(bgra).to(DEV)
    whole = torch.full((guard + n + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    assert whole.data_ptr() % 16 == 0
    out = whole[guard + offset:]
    _convert(src, w, h, w * 4, out)
    got = whole.cpu().numpy()
    assert np.all(got[:guard + offset] == 0xA5) and np.all(got[guard + offset + n:] == 0xA5)
    tensor = got[guard + offset:guard + offset + n].view(np.float32).reshape(h, w, 4)
    assert np.array_equal(_bits(tensor), _bits(tensor_ref.tensor_from_bgra(bgra)))


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("window", [(61, 9, 100), (64, 4, 128), (48, 3, 53)])
def test_pitched_source(window, offset):
    """A window of a wider image: rows pitch_bytes apart; the bytes between them never reach the output."""
    import torch

    w, h, full = window
    rng = np.random.default_rng(w)
    image = rng.integers(0, 256, (h + 2, full, 4), dtype=np.uint8)
    src = torch.from_numpy(image).to(DEV)
    x0, y0 = 4, 1
    first = src[y0:, x0:]
    assert first.data_ptr() == src.data_ptr() + (y0 * full + x0) * 4
    n = 16 * w * h
    whole = torch.full((offset + n + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    _convert(first, w, h, full * 4, whole[offset:])
    got = whole.cpu().numpy()
    assert np.all(got[:offset] == 0xA5) and np.all(got[offset + n:] == 0xA5)
    want = tensor_ref.tensor_from_bgra(image[y0:y0 + h, x0:x0 + w])
    assert np.array_equal(_bits(got[offset:offset + n].view(np.float32).reshape(h, w, 4)), _bits(want))


def test_convert_rejects_bad_arguments(hiplib):
    import torch
    from trident_raster import abi

    src = torch.zeros(64 * 4 + 16, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(64 * 16 + 16, dtype=torch.uint8, device=DEV)
    s, d = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    call = hiplib.tri_convert_rgba_f32
    assert call(s, 8, 8, 32, d, None) == abi.TRI_OK
    for args in [(None, 8, 8, 32, d), (s, 8, 8, 32, None), (s, 0, 8, 32, d), (s, 8, 0, 32, d), (s, 8193, 1, 8193 * 4, d),
                 (s, 1, 8193, 4, d), (s, 8, 8, 28, d), (s, 8, 8, 34, d), (C.c_void_p(src.data_ptr() + 2), 8, 8, 32, d),
                 (s, 8, 8, 32, C.c_void_p(dst.data_ptr() + 2))]:
        assert call(*args, None) == abi.TRI_E_INVALID, args[1:4]
        assert hiplib.tri_last_error()
    torch.cuda.synchronize()


def _frame_tensor(raster_obj):
    col, _ = raster_obj.readback(depth=False)  # BGRA rows
    return tensor_ref.tensor_from_bgra(col)


def _device_floats(ptr, count):
    from trident_raster import raster

    return raster.copy_device_to_host(ptr, 4 * count).view(np.float32)


def test_framegrab_keeps_frames_in_order():
    """Two captures in flight before either is collected: each slot holds its own frame, on the host and on the device."""
    from trident_raster import abi, raster, scenes

    frames = [sc.c1_cube_skybox(f) for f in (0, 1)]
    want = []
    for s in frames:  # the frames' tensors from a separate context
        with raster.TriRaster(s.width, s.height) as ref:
            scenes.load_scene(ref, s)
            ref.render_frame()
            want.append(_frame_tensor(ref))
    assert not np.array_equal(want[0], want[1])
    n = 640 * 480 * 4
    with raster.TriRaster(640, 480) as r, raster.FrameGrab(640, 480, 2, host_copy=True) as grab:
        scenes.load_scene(r, frames[0])
        r.render()
        grab.capture(0, r)
        scenes.load_scene(r, frames[1])
        r.render()
        grab.capture(1, r)
        (h0, d0), (h1, d1) = grab.wait(0), grab.wait(1)
        assert d0 and d1 and d0 != d1
        assert np.array_equal(_bits(h0), _bits(want[0]))
        assert np.array_equal(_bits(h1), _bits(want[1]))
        assert np.array_equal(_bits(_device_floats(d0, n)), _bits(h0).reshape(-1))  # host and device tensors agree
        assert np.array_equal(_bits(_device_floats(d1, n)), _bits(h1).reshape(-1))
        assert grab.wait_pointers(0, host=True, device=False)[1] is None  # either out-pointer may be NULL
        grab.release(0)
        grab.release(1)
        grab.capture(0, r)  # a released slot serves again
        assert np.array_equal(_bits(grab.wait(0)[0]), _bits(want[1]))
        grab.release(0)
        r.synchronize()
    # without the flag the tensor never leaves the device, and asking for the host copy is a state error
    with raster.TriRaster(640, 480) as r, raster.FrameGrab(640, 480, 1) as grab:
        scenes.load_scene(r, frames[0])
        r.render()
        grab.capture(0, r)
        with pytest.raises(raster.TriError) as ei:
            grab.wait_pointers(0, host=True, device=True)
        assert ei.value.code == abi.TRI_E_STATE
        h, d = grab.wait(0)
        assert h is None and d
        assert np.array_equal(_bits(_device_floats(d, n)), _bits(want[0]).reshape(-1))
        grab.release(0)
        r.synchronize()


def test_framegrab_states(hiplib):
    from trident_raster import abi, raster, scenes

    def fails(code, fn, *args, **kw):
        with pytest.raises(raster.TriError) as ei:
            fn(*args, **kw)
        assert ei.value.code == code
        assert hiplib.tri_last_error()

    s = sc.c1_cube_skybox(0)
    with raster.TriRaster(640, 480) as r, raster.FrameGrab(640, 480, 2, host_copy=True) as grab:
        scenes.load_scene(r, s)
        r.render()
        fails(abi.TRI_E_STATE, grab.wait_pointers, 0)  # idle
        grab.capture(0, r)
        fails(abi.TRI_E_STATE, grab.capture, 0, r)  # busy
        fails(abi.TRI_E_INVALID, grab.capture, 2, r)  # slot 2 of 2
        fails(abi.TRI_E_INVALID, grab.wait_pointers, 2)
        fails(abi.TRI_E_INVALID, grab.wait_pointers, 0, host=False, device=False)
        fails(abi.TRI_E_INVALID, grab.release, 2)
        with raster.TriRaster(640, 480, band=(0, 240)) as band:
            fails(abi.TRI_E_STATE, grab.capture, 1, band)
        with raster.TriRaster(320, 240) as small:
            fails(abi.TRI_E_INVALID, grab.capture, 1, small)
        grab.release(0)  # releasing a busy slot waits for its conversion and copy first
        grab.release(0)  # idle: nothing to do
        fails(abi.TRI_E_STATE, grab.wait_pointers, 0)
        r.synchronize()
    import torch

    if torch.cuda.device_count() > 1:  # a context on another device
        with raster.TriRaster(640, 480) as r, raster.FrameGrab(640, 480, 1, device=1) as other:
            scenes.load_scene(r, s)
            r.render()
            fails(abi.TRI_E_INVALID, other.capture, 0, r)
            r.synchronize()
    fails(abi.TRI_E_INVALID, raster.FrameGrab, 640, 480, 1, device=torch.cuda.device_count())
    for slots in (0, 9):
        fails(abi.TRI_E_INVALID, raster.FrameGrab, 640, 480, slots)
    assert hiplib.tri_framegrab_destroy(None) == abi.TRI_OK


# ---- the shim, end to end -------------------------------------------------------------------------------------

W, H = 64, 48


def _scene_app(app_mod, w=W, h=H):
    a = app_mod.TridentApp()
    a.set_camera("editor", (0.0, 1.0, 7.0))
    a.set_viewport(1, w, h)
    cube = a.add_mesh_entity("cube", position=(-0.6, 1.0, -1.0), scale=(2.5, 2.5, 2.5))
    a.add_mesh_entity("sphere", position=(1.4, 0.8, -0.5), scale=(1.8, 1.8, 1.8))
    a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=4.0)
    return a, cube


def _turn(a, cube, f):
    a.set_entity_transform(cube, rotation=(0.0, 23.0 * f, 0.0))


@pytest.fixture(scope="module")
def plain_frames(app_mod):
    """The six frames of the end-to-end runs from a shim that never captures: RGBA8 [6, H, W, 4]. Shared; read only."""
    a, cube = _scene_app(app_mod)
    out = []
    for f in range(6):
        _turn(a, cube, f)
        a.draw_frame()
        out.append(a.read_pixels(1, W, H, depth=False)[0])
    a.close()
    out = np.stack(out)
    assert any(not np.array_equal(out[0], f) for f in out[1:])  # the cube turns
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("in_flight", [1, 3])
def test_shim_records_every_second_tensor(app_mod, tmp_path, plain_frames, in_flight):
    """Throttles 0, interval 2, six frames: three input samples holding the tensors of frames 2, 4 and 6, and the Y4M
    file recorded at the same time is what recording alone writes."""
    a, cube = _scene_app(app_mod)
    a.set_frames_in_flight(in_flight)
    assert a.set_recording(True, 1, W, H, tmp_path / "both.y4m") == (True, (W, H))
    a.set_dataset_capture(True, tmp_path / "cap", 2)
    assert a.set_ai_readback(True, 0, 0)
    tensors = []
    for f in range(6):
        _turn(a, cube, f)
        a.draw_frame()
        a.finish_frame()
        dev = a.readback_device_tensor()
        assert dev is not None and dev[1:] == (W, H)
        resident = _device_floats(dev[0], W * H * 4).reshape(H, W, 4).copy()
        t = a.acquire_frame()
        assert t is not None and t.shape == (H, W, 4)
        assert a.acquire_frame() is None  # handed out once
        assert np.array_equal(_bits(resident), _bits(t))  # the device-resident tensor is the same tensor
        tensors.append(t)
    for t, rgba in zip(tensors, plain_frames):  # the readback-derived tensors: capturing changes no pixel
        assert np.array_equal(_bits(t), _bits(tensor_ref.tensor_from_rgba(rgba)))
    a.set_dataset_capture(False)  # flushes
    assert a.set_recording(False)[0]
    a.close()
    root = tmp_path / "cap"
    assert sorted(p.name for p in (root / "inputs").iterdir()) == ["frame_%06d.npy" % i for i in range(3)]
    assert sorted(p.name for p in (root / "metadata").iterdir()) == ["frame_%06d.json" % i for i in range(3)]
    assert list((root / "outputs").iterdir()) == []
    for i, f in enumerate((1, 3, 5)):  # frames 2, 4 and 6
        assert (root / ("inputs/frame_%06d.npy" % i)).read_bytes() == tensor_ref.npy_bytes(tensors[f], (1, H, W, 4))
        assert np.array_equal(_bits(np.load(root / ("inputs/frame_%06d.npy" % i))), _bits(tensors[f][None]))
        assert (root / ("metadata/frame_%06d.json" % i)).read_text() == tensor_ref.metadata_text(W, H, 4, (1, H, W, 4))
    assert (tmp_path / "both.y4m").read_bytes() == yuv_ref.y4m_file(W, H, 1, list(plain_frames))


def test_shim_pipelined_frames_resolve_late_and_newest_wins(app_mod, plain_frames):
    """Three frames in flight and no fence between them: frame k's DrawFrame fences frame k - 3, whose target it
    reuses, and resolves its tensor; a newer frame replaces an unconsumed one, and FinishFrame brings the last."""
    a, cube = _scene_app(app_mod)
    a.set_frames_in_flight(3)
    assert a.set_ai_readback(True, 0, 0)
    for f in range(5):
        _turn(a, cube, f)
        a.draw_frame()
    t = a.acquire_frame()  # frames 0 and 1 were resolved; 1 replaced the unconsumed 0
    assert np.array_equal(_bits(t), _bits(tensor_ref.tensor_from_rgba(plain_frames[1])))
    assert a.acquire_frame() is None
    a.finish_frame()
    from trident_raster import abi

    small, w, h, got = np.empty(8, np.float32), C.c_uint32(), C.c_uint32(), C.c_int(7)
    rc = a._lib.trident_app_acquire_frame(a._h, small.ctypes.data, small.size, C.byref(w), C.byref(h), C.byref(got))
    assert rc == abi.TRI_E_INVALID and got.value == 0 and (w.value, h.value) == (W, H)  # too small: it stays pending
    buf = np.zeros(W * H * 4 + 5, np.float32)
    t = a.acquire_frame(buf)  # into the caller's buffer
    assert np.shares_memory(t, buf) and buf[-1] == 0
    assert np.array_equal(_bits(t), _bits(tensor_ref.tensor_from_rgba(plain_frames[4])))
    assert a.acquire_frame(buf) is None
    a.close()


def test_shim_present_extent_mismatch_yields_no_tensor(app_mod, plain_frames):
    a, cube = _scene_app(app_mod)
    assert a.set_ai_readback(True, 0, 0)
    a.set_present_extent(W * 2, H * 2)  # the swapchain differs from the viewport: the reference skips the copy
    _turn(a, cube, 0)
    a.draw_frame()
    a.finish_frame()
    assert a.acquire_frame() is None and a.readback_device_tensor() is None
    a.set_present_extent(W, H)  # the same extent: captured
    a.draw_frame()
    a.finish_frame()
    t = a.acquire_frame()
    assert np.array_equal(_bits(t), _bits(tensor_ref.tensor_from_rgba(plain_frames[0])))
    a.set_present_extent(0, 0)
    a.set_viewport(1, W + 16, H)  # a resize rebuilds the grab at the new extent
    a.draw_frame()
    a.finish_frame()
    t = a.acquire_frame()
    rgba = a.read_pixels(1, W + 16, H, depth=False)[0]
    assert t.shape == (H, W + 16, 4) and np.array_equal(_bits(t), _bits(tensor_ref.tensor_from_rgba(rgba)))
    a.close()


def test_shim_ai_output_is_paired_and_blended(app_mod, tmp_path, plain_frames):
    a, cube = _scene_app(app_mod)
    a.set_dataset_capture(True, tmp_path / "cap", 1)
    assert a.set_ai_readback(True, 0, 0)
    _turn(a, cube, 0)
    a.draw_frame()
    a.finish_frame()
    t = a.acquire_frame()
    assert t is not None
    before = a.read_pixels(1, W, H, depth=False)[0]
    assert np.array_equal(before, plain_frames[0])
    rng = np.random.default_rng(9)
    out = rng.integers(0, 256, (H, W, 3)).astype(np.float32)  # a generator that answers in [0, 255], three channels
    assert not a.submit_ai_output(out, (H * W * 3,))  # not NHWC: nothing changes
    assert a.submit_ai_output(out, (-1, H, W, 3))
    a.set_ai_blend_strength(1.0)
    a.draw_frame()
    blended = a.read_pixels(1, W, H, depth=False)[0]
    assert not np.array_equal(blended, before)
    a.set_dataset_capture(False)
    root = tmp_path / "cap"
    want = tensor_ref.normalise_ai_output(out, 3)
    assert (root / "outputs/ai_000000.npy").read_bytes() == tensor_ref.npy_bytes(want, (1, H, W, 3))
    assert (root / "inputs/frame_000000.npy").read_bytes() == tensor_ref.npy_bytes(t, (1, H, W, 4))
    assert sorted(p.name for p in (root / "outputs").iterdir()) == ["ai_000000.npy"]
    # at full strength every mesh pixel is its AI texel: the normalised output (channels 0 and 2 swapped) as UNORM8
    texels = np.round(want.reshape(H, W, 3) * np.float32(255)).astype(np.uint8)
    changed = np.any(blended != before, axis=-1)
    assert changed.sum() > 200
    assert np.array_equal(blended[changed][:, :3], texels[changed])
    a.close()


def test_shim_refuses_readback_on_multi_device_viewports(app_mod):
    a, cube = _scene_app(app_mod)
    assert a.set_ai_readback(True, 0, 0)
    a.draw_frame()
    a.set_device_count(2, [0, 0])  # turns it off
    assert not a.ai_readback_enabled()
    assert not a.set_ai_readback(True, 0, 0)  # and refuses it
    assert not a.ai_readback_enabled()
    a.draw_frame()
    a.finish_frame()
    assert a.acquire_frame() is None
    a.set_device_count(1)
    assert a.set_ai_readback(True, 0, 0)
    a.draw_frame()
    a.finish_frame()
    assert a.acquire_frame() is not None
    a.close()


def test_overflowed_frame_is_captured_again(app_mod):
    """A frame that outgrew the bin queues is re-rendered at its fence; its tensor must hold the re-rendered pixels,
    not the incomplete first attempt's (the scene of test_recording_gpu's test of the same name)."""
    a = app_mod.TridentApp()
    a.set_camera("editor", (0.0, 0.0, 0.0))
    a.set_viewport(1, 1280, 720)
    for k in range(400):
        a.add_mesh_entity("cube", position=(0.0, 0.0, -3.0 - 0.01 * k), rotation=(10.0 * k, 7.0 * k, 0.0),
                          scale=(4.0, 4.0, 4.0))
    assert a.set_ai_readback(True, 0, 0)
    a.draw_frame()
    a.finish_frame()
    t = a.acquire_frame()
    rgba, _ = a.read_pixels(1, 1280, 720, depth=False)
    assert t is not None and np.array_equal(_bits(t), _bits(tensor_ref.tensor_from_rgba(rgba)))
    a.close()
