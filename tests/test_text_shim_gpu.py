"""Renderer::SubmitText through the engine API on the GPU: the label in the viewport's pixels (against a C-ABI render
of the same scene with quads laid out by the trident_font facade), in the recorded Y4M frames, in the AI tensor, per
frame with frames in flight, and dropped for an unknown viewport."""
import os

import numpy as np
import pytest

import scene_cases as sc
import tensor_ref
import yuv_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FONT = os.path.join(ROOT, "tests", "golden", "fonts", "JetBrainsMono-Regular.ttf")
WHITE = (1.0, 1.0, 1.0, 1.0)
CLEAR = (0.1, 0.2, 0.3, 1.0)


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


@pytest.fixture(scope="module")
def faces():
    f = sc.cubemap_faces()
    f.setflags(write=False)
    return f


def _app(app_mod, faces, w, h, vp=1):
    a = app_mod.TridentApp()
    a.set_camera("editor", (0.0, 1.0, 7.0))
    a.set_camera("runtime", (0.5, 1.2, 6.0), (0.0, 5.0, 0.0))
    a.set_viewport(vp, w, h)
    a.set_clear_color(CLEAR)
    a.set_skybox(faces)
    a.add_mesh_entity("cube", position=(-1.2, 1.0, -1.0), scale=(1.5, 1.5, 1.5))
    a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=4.0)
    assert a.set_font(FONT, 32.0)
    assert not a.set_font(FONT + ".missing", 32.0)  # refused: the font above stays
    return a


def test_label_through_the_shim(app_mod, faces):
    from trident_raster import raster, scenes

    w, h = 320, 120
    a = _app(app_mod, faces, w, h)
    a.submit_text(1, (10.0, 30.0), WHITE, "FPS: 123.4")
    a.submit_text(1, (10.0, 70.0), WHITE, "")  # empty text is ignored
    a.draw_frame()
    with_text, depth_text = a.read_pixels(1, w, h)
    a.draw_frame()  # nothing submitted: the queue lasted one frame
    without, depth_plain = a.read_pixels(1, w, h)
    assert np.array_equal(depth_text, depth_plain)
    changed = np.any(with_text != without, axis=-1)
    ys, xs = np.nonzero(changed)
    assert changed.sum() > 300 and xs.min() >= 10 and xs.max() < 10 + 10 * 15 + 2 and ys.min() >= 30 - 26 and ys.max() <= 38

    # the same frames through the C-ABI, the quads from the facade's layout
    font = app_mod.Font(FONT, 32.0)
    quads = font.layout("FPS: 123.4", (10.0, 30.0), WHITE)
    assert quads.shape == (10, 12)
    ubo, draws = a.frame_inputs(1)
    vb, ib, ranges = a.geometry()
    s = scenes.Scene("label", w, h, vb, ib, ranges, draws, ubo, materials=[(m[0], m[1]) for m in a.materials()],
                     skybox=faces, clear=CLEAR)
    with raster.TriRaster(w, h) as r, raster.TriFont(font.atlas()) as atlas:
        scenes.load_scene(r, s)
        r.render_frame()
        plain = r.readback(depth=False)[0][..., [2, 1, 0, 3]]
        r.set_text(atlas, quads)
        r.render_frame()
        label = r.readback(depth=False)[0][..., [2, 1, 0, 3]]
        r.set_text(None, None)
    assert np.array_equal(plain, without)
    diff = np.abs(label.astype(np.int16) - with_text.astype(np.int16))
    print("label through the shim vs the C-ABI: max difference", int(diff.max()), "LSB (expected 0)")
    assert int(diff.max()) <= 1
    a.close()


def _records(path, w, h):
    data = path.read_bytes()
    head = yuv_ref.y4m_header(w, h, 1)
    assert data[:len(head)] == head
    body, size = data[len(head):], 6 + 3 * w * h
    assert len(body) % size == 0
    return [np.frombuffer(body[i + 6:i + size], np.uint8).reshape(3, h, w) for i in range(0, len(body), size)]


def test_recorded_frames_carry_the_text(app_mod, faces, tmp_path):
    w, h = 64, 48
    a = _app(app_mod, faces, w, h)
    assert a.set_recording(True, 1, w, h, tmp_path / "t.y4m") == (True, (w, h))
    frames = []
    for text in ("ab", None, "Zq"):
        if text:
            a.submit_text(1, (4.0, 30.0), (1.0, 0.9, 0.2, 1.0), text)
        a.draw_frame()
        frames.append(a.read_pixels(1, w, h, depth=False)[0])
    assert a.set_recording(False)[0]
    recs = _records(tmp_path / "t.y4m", w, h)
    assert len(recs) == 3
    for rec, f in zip(recs, frames):
        assert np.array_equal(rec, yuv_ref.yuv444(f))
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[0], frames[2])
    assert not np.array_equal(recs[0], recs[1])
    a.close()


def test_ai_tensor_carries_the_text(app_mod, faces):
    w, h = 64, 48
    a = _app(app_mod, faces, w, h)
    assert a.set_ai_readback(True, 0, 0)
    a.draw_frame()
    a.finish_frame()
    plain = a.acquire_frame()
    a.submit_text(1, (4.0, 30.0), WHITE, "AI")
    a.draw_frame()
    a.finish_frame()
    t = a.acquire_frame()
    rgba = a.read_pixels(1, w, h, depth=False)[0]
    assert t is not None and plain is not None and t.shape == (h, w, 4)
    assert np.array_equal(t.view(np.uint32), tensor_ref.tensor_from_rgba(rgba).view(np.uint32))
    assert not np.array_equal(t, plain)
    a.close()


def test_frames_in_flight_keep_their_own_text(app_mod, faces):
    """Three ring targets (separate contexts), four frames with a string each: every frame shows its own."""
    w, h = 200, 48
    strings = ["frame 0", "1 ONE", "two 2 two", "3"]
    a = _app(app_mod, faces, w, h)
    want = []
    for s in strings:  # one frame in flight: the reference
        a.submit_text(1, (6.0, 32.0), WHITE, s)
        a.draw_frame()
        want.append(a.read_pixels(1, w, h, depth=False)[0])
    a.close()
    assert all(not np.array_equal(want[0], f) for f in want[1:])
    b = _app(app_mod, faces, w, h)
    b.set_frames_in_flight(3)
    assert b.set_font(FONT, 32.0)
    for s, f in zip(strings, want):
        b.submit_text(1, (6.0, 32.0), WHITE, s)
        b.draw_frame()
        assert np.array_equal(b.read_pixels(1, w, h, depth=False)[0], f), s
    # nothing read between the frames: the last one still carries its own string
    for s in strings:
        b.submit_text(1, (6.0, 32.0), WHITE, s)
        b.draw_frame()
    assert np.array_equal(b.read_pixels(1, w, h, depth=False)[0], want[-1])
    b.draw_frame()
    assert not np.array_equal(b.read_pixels(1, w, h, depth=False)[0], want[-1])  # no text submitted
    b.close()


def test_text_for_an_unknown_viewport_changes_nothing(app_mod, faces):
    w, h = 96, 48
    a = _app(app_mod, faces, w, h)
    a.draw_frame()
    plain = a.read_pixels(1, w, h, depth=False)[0]
    a.submit_text(7, (4.0, 30.0), WHITE, "nobody")
    a.draw_frame()
    assert np.array_equal(a.read_pixels(1, w, h, depth=False)[0], plain)
    a.draw_frame()  # and it was dropped, not kept for later
    assert np.array_equal(a.read_pixels(1, w, h, depth=False)[0], plain)
    a.close()
