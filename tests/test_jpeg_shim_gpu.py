"""Motion-JPEG recording through the shim on the GPU: Renderer::SetViewportRecordingEnabled with an .mkv path end to end
(the Matroska file a run leaves behind, every block against the numpy restatement of that frame's pixels), the
overflow re-capture, the quality setter and the refusals that stay."""
import os

import numpy as np
import pytest

import jpeg_ref
import mkv_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FONT = os.path.join(ROOT, "tests", "golden", "fonts", "JetBrainsMono-Regular.ttf")


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


def _scene_app(app_mod):
    a = app_mod.TridentApp()
    a.set_camera("editor", (0.0, 1.0, 7.0))
    a.set_viewport(1, 161, 99)
    cube = a.add_mesh_entity("cube", position=(-1.2, 1.0, -1.0), scale=(1.5, 1.5, 1.5))
    a.add_mesh_entity("sphere", position=(1.4, 0.8, -0.5), scale=(1.8, 1.8, 1.8))
    a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=4.0)
    return a, cube


def _bgra(rgba):
    return np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])


def _blocks(path, w, h, count):
    m = mkv_ref.parse(open(path, "rb").read())
    assert m["complete"] and m["segment_size_known"] and m["track"]["CodecID"] == "V_MJPEG"
    assert (m["track"]["PixelWidth"], m["track"]["PixelHeight"]) == (w, h)
    assert len(m["blocks"]) == count and all(b["flags"] == 0x80 for b in m["blocks"])
    return [b["data"] for b in m["blocks"]]


def test_shim_records_every_frame_to_matroska(app_mod, tmp_path):
    a, cube = _scene_app(app_mod)
    assert a.set_font(FONT, 24.0)
    a.set_frames_in_flight(2)
    assert a.set_recording_quality(80) == 80
    ok, extent = a.set_recording(True, 1, 161, 99, tmp_path / "a.MKV")
    assert ok and extent == (162, 100)  # odd sides rounded up to even; the encoder pads to 16 itself
    frames = []
    for f in range(5):
        a.set_entity_transform(cube, rotation=(0.0, 23.0 * f, 0.0))
        a.submit_text(1, (8.0, 30.0), (1.0, 0.9, 0.2, 1.0), f"frame {f}")
        a.draw_frame()
        frames.append(a.read_pixels(1, 162, 100, depth=False)[0])
    assert a.recording_state() == (True, 5)
    assert a.set_recording(False)[0] and a.recording_state() == (False, 5)
    assert any(not np.array_equal(frames[0], f) for f in frames[1:])
    blocks = _blocks(tmp_path / "a.MKV", 162, 100, 5)
    for got, f in zip(blocks, frames):
        assert got == jpeg_ref.encode(_bgra(f), 80, 0)
    # the host encoder writes the same file from those frames
    enc = app_mod.VideoEncoder()
    assert enc.set_quality(80) and enc.begin(tmp_path / "host.mkv", 162, 100, 1)
    for f in frames:
        assert enc.submit_rgba(f, 162, 100)
    assert enc.end()
    assert (tmp_path / "host.mkv").read_bytes() == (tmp_path / "a.MKV").read_bytes()
    # the quality is clamped and applies from the next session; .y4m is exactly what it was
    assert a.set_recording_quality(0) == 1 and a.set_recording_quality(1000) == 100 and a.set_recording_quality(35) == 35
    assert a.set_recording(True, 1, 162, 100, tmp_path / "b.mkv")[0]
    a.draw_frame()
    rgba = a.read_pixels(1, 162, 100, depth=False)[0]
    assert a.set_recording(True, 1, 162, 100, tmp_path / "c.y4m")[0]  # a restart finalises the running file
    assert _blocks(tmp_path / "b.mkv", 162, 100, 1)[0] == jpeg_ref.encode(_bgra(rgba), 35, 0)
    a.draw_frame()
    assert a.set_recording(False)[0]
    assert os.path.getsize(tmp_path / "c.y4m") > 3 * 162 * 100
    # the refusals are unchanged
    for name in ("a.mp4", "a.avi", "a.bin"):
        assert not a.set_recording(True, 1, 162, 100, tmp_path / name)[0] and not (tmp_path / name).exists()
    a.set_device_count(2, [0, 0])
    assert not a.set_recording(True, 1, 162, 100, tmp_path / "multi.mkv")[0] and not (tmp_path / "multi.mkv").exists()
    a.close()


def test_destroyed_while_recording_matroska(app_mod, tmp_path):
    b, cube = _scene_app(app_mod)
    b.set_frames_in_flight(3)
    assert b.set_recording(True, 1, 160, 96, tmp_path / "t.mkv") == (True, (160, 96))
    for f in range(4):
        b.set_entity_transform(cube, rotation=(0.0, 11.0 * f, 0.0))
        b.draw_frame()
    b.close()  # frames still in flight: the file is complete and its sizes are patched
    assert len(_blocks(tmp_path / "t.mkv", 160, 96, 4)) == 4


def test_overflowed_frame_is_captured_again_as_jpeg(app_mod, tmp_path):
    """A frame that outgrew the bin queues is re-rendered at its fence; its block must hold the re-rendered pixels."""
    from trident_raster import abi, raster

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
    assert a.set_recording(True, 1, 1280, 720, tmp_path / "o.mkv") == (True, (1280, 720))
    a.draw_frame()
    rgba, _ = a.read_pixels(1, 1280, 720, depth=False)
    assert a.set_recording(False)[0]
    blocks = _blocks(tmp_path / "o.mkv", 1280, 720, 1)
    assert blocks[0] == jpeg_ref.encode(_bgra(rgba), 90, 0)
    a.close()
