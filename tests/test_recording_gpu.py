"""Viewport recording on the GPU: k_bgra_to_yuv444 (tri_convert_yuv444) against the float64 restatement with zero
differing bytes, the tri_recorder slot protocol, and Renderer::SetViewportRecordingEnabled end to end through the
shim (the Y4M file a run leaves behind, byte for byte)."""
import ctypes as C

import numpy as np
import pytest

import scene_cases as sc
import yuv_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


def _convert(src, width, height, pitch, dst):
    import torch
    from trident_raster import raster

    raster.convert_yuv444(src.data_ptr(), width, height, pitch, dst.data_ptr())  # the null stream, as torch's
    torch.cuda.synchronize()


def test_every_triple_matches_the_restatement():
    import torch

    rgb, want = yuv_ref.all_triples()
    bgra = np.empty((1 << 24, 4), np.uint8)  # a 4096 x 4096 image holding every triple once
    bgra[:, 0], bgra[:, 1], bgra[:, 2] = rgb[:, 2], rgb[:, 1], rgb[:, 0]
    bgra[:, 3] = rgb[:, 0] ^ rgb[:, 1] ^ rgb[:, 2]
    src = torch.from_numpy(bgra).to(DEV)
    dst = torch.zeros(3 << 24, dtype=torch.uint8, device=DEV)
    _convert(src, 4096, 4096, 4096 * 4, dst)
    got = dst.cpu().numpy().reshape(3, 1 << 24)
    for k, name in enumerate("YUV"):
        assert int((got[k] != want[k]).sum()) == 0, name


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", [(1, 1), (3, 1), (5, 3), (7, 5), (64, 1), (65, 2), (130, 3), (1023, 2), (4099, 3)])
def test_ragged_shapes_and_guard_bytes(shape, offset):
    """Widths that are no multiple of the 16-pixel run, planes that start on odd addresses (width * height odd, or
    the destination one byte into its tensor): the output is exact and nothing around it is written."""
    import torch

    w, h = shape
    rng = np.random.default_rng(1000 * w + 10 * h + offset)
    bgra = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    n, guard = 3 * w * h, 64
    src = torch.from_numpy(bgra).to(DEV)
    whole = torch.full((offset + n + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    _convert(src, w, h, w * 4, whole[offset:])
    got = whole.cpu().numpy()
    assert np.all(got[:offset] == 0xA5) and np.all(got[offset + n:] == 0xA5)
    assert np.array_equal(got[offset:offset + n].reshape(3, h, w), yuv_ref.yuv444(bgra[..., [2, 1, 0]]))


@pytest.mark.parametrize("window", [(61, 9, 100), (64, 4, 128), (48, 3, 53)])
def test_pitched_source(window):
    """A window of a wider image: rows pitch_bytes apart, the bytes between them never reach the output. 61 x 9 of
    100: every plane row starts at another alignment; 64 x 4 of 128: every run is whole and 16-B aligned; 48 x 3 of
    53: whole runs whose source rows (212 B apart) are only 4-B aligned beyond the first."""
    import torch

    w, h, full = window
    rng = np.random.default_rng(w)
    image = rng.integers(0, 256, (h + 2, full, 4), dtype=np.uint8)
    src = torch.from_numpy(image).to(DEV)
    x0, y0 = 4, 1  # (x0 * 4 = 16: the window's first row starts 16-B aligned when `full` allows)
    first = src[y0:, x0:]
    assert first.data_ptr() == src.data_ptr() + (y0 * full + x0) * 4
    whole = torch.full((3 * w * h + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    _convert(first, w, h, full * 4, whole)
    got = whole.cpu().numpy()
    assert np.all(got[3 * w * h:] == 0xA5)
    want = yuv_ref.yuv444(image[y0:y0 + h, x0:x0 + w][..., [2, 1, 0]])
    assert np.array_equal(got[:3 * w * h].reshape(3, h, w), want)


def test_convert_rejects_bad_arguments(hiplib):
    import torch
    from trident_raster import abi

    src = torch.zeros(64 * 4 + 16, dtype=torch.uint8, device=DEV)
    dst = torch.zeros(3 * 64, dtype=torch.uint8, device=DEV)
    s, d = C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())
    call = hiplib.tri_convert_yuv444
    assert call(s, 8, 8, 32, d, None) == abi.TRI_OK
    for args in [(None, 8, 8, 32, d), (s, 8, 8, 32, None), (s, 0, 8, 32, d), (s, 8, 0, 32, d), (s, 8193, 1, 8193 * 4, d),
                 (s, 1, 8193, 4, d), (s, 8, 8, 28, d), (s, 8, 8, 34, d), (C.c_void_p(src.data_ptr() + 2), 8, 8, 32, d)]:
        assert call(*args, None) == abi.TRI_E_INVALID, args[1:4]
        assert hiplib.tri_last_error()
    torch.cuda.synchronize()


def _frame_rgb(raster_obj):
    col, _ = raster_obj.readback(depth=False)  # BGRA rows
    return col[..., [2, 1, 0]]


def test_recorder_keeps_frames_in_order():
    """Two captures in flight before either is collected: each slot holds its own frame."""
    from trident_raster import raster, scenes

    frames = [sc.c1_cube_skybox(f) for f in (0, 1)]
    want = []
    for s in frames:  # the frames' colours from a separate context
        with raster.TriRaster(s.width, s.height) as ref:
            scenes.load_scene(ref, s)
            ref.render_frame()
            want.append(yuv_ref.yuv444(_frame_rgb(ref)))
    assert not np.array_equal(want[0], want[1])
    with raster.TriRaster(640, 480) as r, raster.TriRecorder(640, 480, 2) as rec:
        scenes.load_scene(r, frames[0])
        r.render()
        rec.capture(0, r)
        scenes.load_scene(r, frames[1])
        r.render()
        rec.capture(1, r)
        p0, p1 = rec.wait_pointer(0), rec.wait_pointer(1)
        assert p0 and p1 and p0 != p1
        assert np.array_equal(rec.wait(0), want[0])
        assert np.array_equal(rec.wait(1), want[1])
        rec.release(0)
        rec.release(1)
        rec.capture(0, r)  # a released slot serves again
        assert np.array_equal(rec.wait(0), want[1])
        rec.release(0)
        r.synchronize()


def test_recorder_states(hiplib):
    from trident_raster import abi, raster, scenes

    def fails(code, fn, *args):
        with pytest.raises(raster.TriError) as ei:
            fn(*args)
        assert ei.value.code == code
        assert hiplib.tri_last_error()

    s = sc.c1_cube_skybox(0)
    with raster.TriRaster(640, 480) as r, raster.TriRecorder(640, 480, 2) as rec:
        scenes.load_scene(r, s)
        r.render()
        fails(abi.TRI_E_STATE, rec.wait_pointer, 0)  # idle
        rec.capture(0, r)
        fails(abi.TRI_E_STATE, rec.capture, 0, r)  # busy
        fails(abi.TRI_E_INVALID, rec.capture, 2, r)  # slot 2 of 2
        fails(abi.TRI_E_INVALID, rec.wait_pointer, 2)
        fails(abi.TRI_E_INVALID, rec.release, 2)
        with raster.TriRaster(640, 480, band=(0, 240)) as band:
            fails(abi.TRI_E_STATE, rec.capture, 1, band)
        with raster.TriRaster(320, 240) as small:
            fails(abi.TRI_E_INVALID, rec.capture, 1, small)
        rec.release(0)  # releasing a busy slot waits for its copy first
        rec.release(0)  # idle: nothing to do
        fails(abi.TRI_E_STATE, rec.wait_pointer, 0)
        r.synchronize()
    for slots in (0, 9):
        fails(abi.TRI_E_INVALID, raster.TriRecorder, 640, 480, slots)
    assert hiplib.tri_recorder_destroy(None) == abi.TRI_OK


def test_rings_are_destroyed_with_captures_in_flight(hiplib):
    """The documented teardown (Renderer::StopRecording, Renderer::DropGrab): a recorder, a grab with the host copy and a
    grab without it are destroyed behind two captures that nobody waited for or released. The context is unharmed: it
    synchronises, and its next frame is the one a fresh context renders."""
    from trident_raster import abi, raster, scenes

    frames = [sc.c1_cube_skybox(f) for f in (0, 1)]
    with raster.TriRaster(640, 480) as fresh:
        scenes.load_scene(fresh, frames[1])
        fresh.render_frame()
        want_col, want_dep = fresh.readback()
    rings = [(lambda: raster.TriRecorder(640, 480, 2), "_r", hiplib.tri_recorder_destroy),
             (lambda: raster.FrameGrab(640, 480, 2, host_copy=True), "_g", hiplib.tri_framegrab_destroy),
             (lambda: raster.FrameGrab(640, 480, 2), "_g", hiplib.tri_framegrab_destroy)]
    for make, attr, destroy in rings:
        with raster.TriRaster(640, 480) as r:
            ring = make()
            for slot, s in enumerate(frames):
                scenes.load_scene(r, s)
                r.render()
                ring.capture(slot, r)
            handle = getattr(ring, attr)
            setattr(ring, attr, None)  # the wrapper must not destroy it again
            assert destroy(handle) == abi.TRI_OK
            r.synchronize()
            r.render_frame()
            col, dep = r.readback()
            assert np.array_equal(col, want_col) and np.array_equal(dep, want_dep)


# ---- the shim, end to end -------------------------------------------------------------------------------------

def _scene_app(app_mod, w1=321, h1=201):
    a = app_mod.TridentApp()
    a.set_camera("editor", (0.0, 1.0, 7.0))
    a.set_camera("runtime", (0.5, 1.2, 6.0), (0.0, 5.0, 0.0))
    a.set_viewport(2, 160, 100)
    a.set_viewport(1, w1, h1)
    cube = a.add_mesh_entity("cube", position=(-1.2, 1.0, -1.0), scale=(1.5, 1.5, 1.5))
    a.add_mesh_entity("sphere", position=(1.4, 0.8, -0.5), scale=(1.8, 1.8, 1.8))
    a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=4.0)
    return a, cube


def _run(a, cube, frames, read_each):
    out = []
    for f in range(frames):
        a.set_entity_transform(cube, rotation=(0.0, 23.0 * f, 0.0))
        a.draw_frame()
        if read_each:
            out.append(a.read_pixels(1, 322, 202, depth=False)[0])
    return out


def _split(data, w, h):
    head = yuv_ref.y4m_header(w, h, 1)  # SetViewportRecordingEnabled starts the session with fps 1
    assert data[:len(head)] == head
    body, size = data[len(head):], 6 + 3 * w * h
    assert len(body) % size == 0
    return [body[i:i + size] for i in range(0, len(body), size)]


def test_shim_records_every_frame(app_mod, tmp_path):
    a, cube = _scene_app(app_mod)
    ok, extent = a.set_recording(True, 1, 321, 201, tmp_path / "a.y4m")
    assert ok and extent == (322, 202)  # odd sides rounded up
    assert a.recording_state() == (True, 0)
    frames = _run(a, cube, 5, read_each=True)
    img = a.viewport_texture(1)
    assert (img.width, img.height) == (322, 202)
    img2 = a.viewport_texture(2)
    assert (img2.width, img2.height) == (160, 100)  # the other viewport keeps its size
    a.set_viewport(1, 300, 180)  # the layout cannot shrink the recorded viewport
    a.set_viewport(1, 321, 201)
    assert a.set_recording(False)[0]
    assert a.recording_state() == (False, 5)
    data = (tmp_path / "a.y4m").read_bytes()
    recs = _split(data, 322, 202)
    assert len(recs) == 5
    assert any(not np.array_equal(frames[0], f) for f in frames[1:])  # the cube turns
    for rec, f in zip(recs, frames):
        assert rec[:6] == b"FRAME\n"
        assert np.array_equal(np.frombuffer(rec[6:], np.uint8).reshape(3, 202, 322), yuv_ref.yuv444(f))
    # the same file from the host encoder fed with those RGBA frames
    enc = app_mod.VideoEncoder()
    assert enc.begin(tmp_path / "host.y4m", 322, 202, 1)
    for f in frames:
        assert enc.submit_rgba(f, 322, 202)
    assert enc.end()
    assert (tmp_path / "host.y4m").read_bytes() == data
    a.close()

    # three frames in flight, nothing read per frame: the same bytes
    b, cube = _scene_app(app_mod)
    b.set_frames_in_flight(3)
    assert b.set_recording(True, 1, 321, 201, tmp_path / "b.y4m") == (True, (322, 202))
    _run(b, cube, 5, read_each=False)
    b.finish_frame()
    assert b.recording_state() == (True, 5)
    assert b.set_recording(False)[0]
    assert (tmp_path / "b.y4m").read_bytes() == data
    b.close()

    # recording changes no pixel: the same frames from a 322 x 202 viewport that was never recorded
    c, cube = _scene_app(app_mod, 322, 202)
    plain = _run(c, cube, 5, read_each=True)
    for f, g in zip(frames, plain):
        assert np.array_equal(f, g)
    assert c.recording_state() == (False, 0)
    c.close()


def test_shim_refusals_and_teardown(app_mod, tmp_path):
    a, cube = _scene_app(app_mod)
    a.draw_frame()
    ok, _ = a.set_recording(True, 1, 321, 201, tmp_path / "a.mp4")
    assert not ok and a.recording_state()[0] is False
    assert not (tmp_path / "a.mp4").exists()
    a.draw_frame()
    img = a.viewport_texture(1)
    assert (img.width, img.height) == (321, 201)  # a refused start resized nothing
    a.set_device_count(2, [0, 0])
    ok, _ = a.set_recording(True, 1, 321, 201, tmp_path / "multi.y4m")
    assert not ok and a.recording_state()[0] is False
    assert not (tmp_path / "multi.y4m").exists()
    a.close()

    b, cube = _scene_app(app_mod)
    b.set_frames_in_flight(2)
    assert b.set_recording(True, 1, 320, 200, tmp_path / "t.y4m") == (True, (320, 200))
    _run(b, cube, 3, read_each=False)
    b.close()  # destroyed while recording, frames still in flight: the file is complete
    size = (tmp_path / "t.y4m").stat().st_size
    assert size == len(yuv_ref.y4m_header(320, 200, 1)) + 3 * (6 + 3 * 320 * 200)


def test_overflowed_frame_is_captured_again(app_mod, tmp_path):
    """A frame that outgrew the bin queues is re-rendered at its fence; its record must hold the re-rendered pixels,
    not the incomplete first attempt's."""
    from trident_raster import abi, raster, scenes

    a = app_mod.TridentApp()
    a.set_camera("editor", (0.0, 0.0, 0.0))
    a.set_viewport(1, 1280, 720)
    for k in range(400):  # the overlapping scale-4 cubes of test_bin_overflow_grows_and_recovers
        a.add_mesh_entity("cube", position=(0.0, 0.0, -3.0 - 0.01 * k), rotation=(10.0 * k, 7.0 * k, 0.0),
                          scale=(4.0, 4.0, 4.0))
    ubo, draws = a.frame_inputs(1)
    vb, ib, ranges = a.geometry()
    with raster.TriRaster(1280, 720) as r:  # the same frame on a fresh context does overflow
        r.upload_geometry(vb, ib, ranges)
        r.upload_materials(a.materials())
        r.set_frame(ubo)
        r.set_draws(draws)
        r.render()
        with pytest.raises(raster.TriError) as ei:
            r.synchronize()
        assert ei.value.code == abi.TRI_E_OVERFLOW
    assert a.set_recording(True, 1, 1280, 720, tmp_path / "o.y4m") == (True, (1280, 720))
    a.draw_frame()
    rgba, _ = a.read_pixels(1, 1280, 720, depth=False)
    assert a.set_recording(False)[0]
    recs = _split((tmp_path / "o.y4m").read_bytes(), 1280, 720)
    assert len(recs) == 1
    assert np.array_equal(np.frombuffer(recs[0][6:], np.uint8).reshape(3, 720, 1280), yuv_ref.yuv444(rgba))
    a.close()
