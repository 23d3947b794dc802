"""Motion vectors through the engine API on the GPU: Renderer::SetMotionVectorOutputEnabled, ReadViewportMotionVectors and
GetViewportMotionTexture over a cube, a sphere, a hidden cube and a sprite in two viewports, with frames in flight, and
refused on multi-device viewports.

The expected motion is tests/motion_ref.py's float32 restatement over the table tri_motion_matrices builds from the
frames' own inputs (trident_app_frame_inputs of the frame and of the one before it, joined per entity as the shim
documents: an entity the last frame did not draw keeps its current model) and the viewport's own ids and depth. Compared
as uint32: zero mismatches."""
import numpy as np
import pytest

import motion_ref as mr
from test_id_shim_gpu import NONE, VIEWPORTS, make_app

pytestmark = pytest.mark.gpu
F = np.float32
ALL = ("cube", "hidden", "sphere", "sprite")
VISIBLE = ("cube", "sphere", "sprite")


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def inputs(a, ents, vp, names):
    """(ubo, draws, {entity: model}) of the viewport's next frame; names: the entities it draws, in draw order."""
    ubo, draws = a.frame_inputs(vp)
    assert len(draws) == len(names)
    return ubo, draws, {ents[n]: np.array(d.pc.model[:], F) for n, d in zip(names, draws)}


def expected(a, ents, vp, size, now, before, names):
    """The restatement for the viewport's latest frame, rendered from `now` with `before` as the frame ahead of it
    (None: no history)."""
    from trident_raster import raster

    w, h = size
    ubo, draws, _ = now
    hist = None
    if before is not None:
        v, p = mr.camera_of(before[0])
        prev = np.array([before[2].get(ents[n], np.array(d.pc.model[:], F)) for n, d in zip(names, draws)], F)
        hist = (v, p, prev)
    table = raster.motion_matrices(ubo, draws, hist)
    entity = a.read_entity_ids(vp, w, h)
    assert entity is not None  # the motion output turned the id output on
    ids = np.zeros((h, w), np.uint32)
    for d, n in enumerate(names):
        ids[entity == ents[n]] = d + 1
    assert ((ids != 0) == (entity != NONE)).all()
    _, depth = a.read_pixels(vp, w, h)
    return mr.restate(table, ids, depth.view(np.uint32), w, h), ids


def check(tag, a, vp, size, want):
    w, h = size
    got = a.read_motion_vectors(vp, w, h)
    assert got is not None, tag
    bad = int((bits(got) != bits(want)).any(axis=-1).sum())
    print(f"SHIM MOTION {tag}: max |m| {np.abs(want).max():.2f} px, {bad} mismatches")
    assert bad == 0, tag
    img = a.motion_texture(vp)
    assert img is not None and (img.width, img.height, img.pitch_bytes, img.format) == (w, h, w * 8, 103) and img.device_ptr
    return got


def test_motion_in_two_viewports(app_mod):
    a, ents = make_app(app_mod)
    a.draw_frame()
    assert a.read_motion_vectors(1, *VIEWPORTS[1]) is None and a.motion_texture(1) is None  # not asked for yet
    for vp in VIEWPORTS:
        assert a.set_motion_vector_output(vp, True)
    first = {vp: inputs(a, ents, vp, VISIBLE) for vp in VIEWPORTS}
    a.draw_frame()
    for vp, size in VIEWPORTS.items():  # frame 1 has no history
        want, _ = expected(a, ents, vp, size, first[vp], None, VISIBLE)
        assert not bits(want).any()
        check(f"viewport {vp} frame 1", a, vp, size, want)
    # the cube and the editor camera move, the hidden cube appears
    a.set_entity_transform(ents["cube"], position=(-1.1, 1.15, -1.0), rotation=(20.0, 38.0, 4.0))
    a.set_camera("editor", (0.2, 1.05, 6.8), (1.0, -2.0, 0.0), far=60.0)
    a.set_entity_visible(ents["hidden"], True)
    second = {vp: inputs(a, ents, vp, ALL) for vp in VIEWPORTS}
    a.draw_frame()
    for vp, size in VIEWPORTS.items():
        want, ids = expected(a, ents, vp, size, second[vp], first[vp], ALL)
        got = check(f"viewport {vp} frame 2", a, vp, size, want)
        cube, hidden, still = ids == 1, ids == 2, (ids == 0) | (ids == 3) | (ids == 4)
        assert cube.any() and hidden.any() and np.abs(got[cube]).max() >= 2.0
        if vp == 2:  # the runtime camera did not move: still entities, the background and the new entity read 0
            assert not bits(got[still]).any() and not bits(got[hidden]).any()
        else:        # under the moved editor camera the new entity takes the camera's motion alone
            from trident_raster import raster

            v, p = mr.camera_of(first[vp][0])
            cam_only = raster.motion_matrices(second[vp][0], second[vp][1], (v, p, None))
            _, depth = a.read_pixels(vp, *size)
            alone = mr.restate(cam_only, ids, depth.view(np.uint32), *size)
            assert np.array_equal(bits(got[hidden]), bits(alone[hidden])) and np.abs(got[hidden]).max() > 0.5
            assert np.abs(got[still]).max() > 0.5
    # a resize: the first frame at the new size has no history, the next one has
    a.set_viewport(1, 80, 50)
    third = inputs(a, ents, 1, ALL)
    a.draw_frame()
    assert not bits(a.read_motion_vectors(1, 80, 50)).any()
    a.set_camera("editor", (0.3, 1.0, 6.7), (1.0, -1.0, 0.0), far=60.0)
    fourth = inputs(a, ents, 1, ALL)
    a.draw_frame()
    want, _ = expected(a, ents, 1, (80, 50), fourth, third, ALL)
    check("viewport 1 after a resize", a, 1, (80, 50), want)
    assert np.abs(want).max() >= 1.0
    # off: the readers answer no more; on again: no history
    assert a.set_motion_vector_output(1, False)
    a.draw_frame()
    assert a.read_motion_vectors(1, 80, 50) is None and a.motion_texture(1) is None
    assert a.set_motion_vector_output(1, True)
    a.draw_frame()
    assert not bits(a.read_motion_vectors(1, 80, 50)).any()
    assert a.read_motion_vectors(9, 4, 4) is None  # no such viewport
    a.close()


def test_motion_with_two_frames_in_flight(app_mod):
    """The history is the viewport's, not the ring target's: frame k is held against frame k - 1, which the other
    target rendered."""
    a, ents = make_app(app_mod, {1: VIEWPORTS[1]})
    a.set_frames_in_flight(2)
    assert a.set_motion_vector_output(1, True)
    size = VIEWPORTS[1]
    before = None
    for k in range(3):
        a.set_entity_transform(ents["cube"], position=(-1.4 + 0.3 * k, 1.0, -1.0))
        a.set_camera("editor", (0.1 * k, 1.0, 7.0 - 0.1 * k), (0.0, 1.5 * k, 0.0), far=60.0)
        now = inputs(a, ents, 1, VISIBLE)
        a.draw_frame()
        want, _ = expected(a, ents, 1, size, now, before, VISIBLE)
        check(f"in flight, frame {k}", a, 1, size, want)
        assert bits(want).any() == (k > 0)
        before = now
    a.close()


def test_multi_device_viewports_refuse_motion(app_mod, capfd):
    a, ents = make_app(app_mod, {1: VIEWPORTS[1]})
    assert a.set_motion_vector_output(1, True)
    a.draw_frame()
    assert a.read_motion_vectors(1, *VIEWPORTS[1]) is not None
    capfd.readouterr()
    a.set_device_count(2, [0, 0])  # turns the output off, and says so
    assert "motion vectors" in capfd.readouterr().err
    a.draw_frame()
    assert a.read_motion_vectors(1, *VIEWPORTS[1]) is None
    assert not a.set_motion_vector_output(1, True)  # refused, with a log line
    assert "motion vectors" in capfd.readouterr().err
    a.draw_frame()
    assert a.read_motion_vectors(1, *VIEWPORTS[1]) is None and a.motion_texture(1) is None
    a.close()
