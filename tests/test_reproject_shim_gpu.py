"""History reprojection through the engine API on the GPU: Renderer::SetHistoryReprojectionEnabled,
ReadViewportReprojection, GetViewportReprojectedTexture and GetViewportDisocclusionTexture over a cube, a sphere and a
sprite in two viewports, across a resize, with frames in flight, and refused on multi-device viewports.

The expected images are tests/reproject_ref.py's float32 restatement over the table tri_motion_matrices builds from the
frames' own inputs (as tests/test_motion_shim_gpu.py joins them per entity) and the viewport's own colour, ids and depth
of the frame and of the one before it. Compared as bytes: zero mismatches."""
import numpy as np
import pytest

import motion_ref as mr
import reproject_ref as rr
from test_id_shim_gpu import NONE, VIEWPORTS, make_app
from test_motion_shim_gpu import VISIBLE, inputs

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


def frame_of(a, ents, vp, size, names):
    """(ids, depth bits, colour B G R A) of the viewport's latest frame; ids are draw ids in `names`' order."""
    w, h = size
    entity = a.read_entity_ids(vp, w, h)
    assert entity is not None  # the request turned the id output on
    ids = np.zeros((h, w), np.uint32)
    for d, n in enumerate(names):
        ids[entity == ents[n]] = d + 1
    assert ((ids != 0) == (entity != NONE)).all()
    rgba, depth = a.read_pixels(vp, w, h)
    return ids, np.ascontiguousarray(depth).view(np.uint32), np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])


def check(tag, a, ents, vp, size, names, now, before, prev):
    """The viewport's reprojection against the restatement; `now` / `before`: test_motion_shim_gpu.inputs of the frame
    and of the one ahead of it (None: no history), prev: that frame's frame_of. Returns (frame_of, warped, mask)."""
    from trident_raster import abi, raster

    w, h = size
    cur = frame_of(a, ents, vp, size, names)
    ubo, draws, _ = now
    hist = None
    if before is not None:
        v, p = mr.camera_of(before[0])
        hist = (v, p, np.array([before[2].get(ents[n], np.array(d.pc.model[:], F)) for n, d in zip(names, draws)], F))
    table = raster.motion_matrices(ubo, draws, hist)
    want_c, want_m = rr.restate(table, cur[0], cur[1], cur[2], prev if before is not None else None, w, h)
    got = a.read_reprojection(vp, w, h)
    assert got is not None, tag
    bad_m, bad_c = int((got[1] != want_m).sum()), int((got[0] != want_c).any(axis=-1).sum())
    print(f"SHIM REPROJECT {tag}: valid {int((want_m == 0).sum())}, outside {int((want_m == 4).sum())}, id "
          f"{int((want_m == 8).sum())}, mask mismatches {bad_m}, colour mismatches {bad_c}")
    assert bad_m == 0 and bad_c == 0, tag
    tex = a.reprojection_textures(vp)
    assert tex is not None
    assert (tex[0].width, tex[0].height, tex[0].pitch_bytes, tex[0].format) == (w, h, w * 4, abi.TRI_FORMAT_B8G8R8A8_UNORM)
    assert (tex[1].width, tex[1].height, tex[1].pitch_bytes, tex[1].format) == (w, h, w, abi.TRI_FORMAT_R8_UINT)
    assert tex[0].device_ptr and tex[1].device_ptr
    return cur, got[0], got[1]


def move(a, ents, k):
    a.set_entity_transform(ents["cube"], position=(-1.4 + 0.3 * k, 1.0, -1.0), rotation=(5.0 * k, 20.0, 0.0))
    a.set_camera("editor", (0.1 * k, 1.0, 7.0 - 0.1 * k), (0.0, 1.5 * k, 0.0), far=60.0)


def test_two_viewports_have_their_own_history_and_a_resize_starts_anew(app_mod):
    a, ents = make_app(app_mod)
    a.draw_frame()
    assert a.read_reprojection(1, *VIEWPORTS[1]) is None and a.reprojection_textures(1) is None  # not asked for yet
    assert not a.set_history_reprojection(1, True, -1.0) and not a.set_history_reprojection(1, True, float("nan"))  # refused
    for vp in VIEWPORTS:
        assert a.set_history_reprojection(vp, True)
    state = {}
    for k in range(3):
        move(a, ents, k)
        now = {vp: inputs(a, ents, vp, VISIBLE) for vp in VIEWPORTS}
        a.draw_frame()
        for vp, size in VIEWPORTS.items():
            before, prev = state.get(vp, (None, None))
            cur, c, m = check(f"viewport {vp} frame {k}", a, ents, vp, size, VISIBLE, now[vp], before, prev)
            if k == 0:
                assert (m == rr.NO_HISTORY).all() and np.array_equal(c, cur[2])
            else:
                assert (m == 0).any() and (m != 0).any()
            state[vp] = (now[vp], cur)
    # a resize: the first frame at the new size has no history, the next one has; the other viewport keeps its own
    a.set_viewport(1, 80, 50)
    sizes = {1: (80, 50), 2: VIEWPORTS[2]}
    state.pop(1)
    for k in (3, 4):
        move(a, ents, k)
        now = {vp: inputs(a, ents, vp, VISIBLE) for vp in sizes}
        a.draw_frame()
        for vp, size in sizes.items():
            before, prev = state.get(vp, (None, None))
            cur, c, m = check(f"viewport {vp} frame {k}", a, ents, vp, size, VISIBLE, now[vp], before, prev)
            assert (m == rr.NO_HISTORY).all() == (vp == 1 and k == 3)
            state[vp] = (now[vp], cur)
    # off: the readers answer no more; on again: no history once
    assert a.set_history_reprojection(1, False)
    a.draw_frame()
    assert a.read_reprojection(1, 80, 50) is None and a.reprojection_textures(1) is None
    assert a.set_history_reprojection(1, True)
    a.draw_frame()
    assert (a.read_reprojection(1, 80, 50)[1] == rr.NO_HISTORY).all()
    a.draw_frame()
    assert (a.read_reprojection(1, 80, 50)[1] == 0).all()  # nothing moved since
    assert a.read_reprojection(9, 4, 4) is None  # no such viewport
    a.close()


def run_in_flight(app_mod, n):
    a, ents = make_app(app_mod, {1: VIEWPORTS[1]})
    a.set_frames_in_flight(n)
    assert a.set_history_reprojection(1, True, 1e-3)
    out = []
    for k in range(4):
        move(a, ents, k)
        a.draw_frame()
        got = a.read_reprojection(1, *VIEWPORTS[1])
        assert got is not None
        out.append(got)
    a.close()
    return out


def test_two_frames_in_flight_equal_one(app_mod):
    """The history is the viewport's, not the ring target's: frame k is warped from frame k - 1, which the other target
    rendered."""
    a, ents = make_app(app_mod, {1: VIEWPORTS[1]})
    a.set_frames_in_flight(2)
    assert a.set_history_reprojection(1, True)
    before, prev = None, None
    for k in range(3):
        move(a, ents, k)
        now = inputs(a, ents, 1, VISIBLE)
        a.draw_frame()
        prev, _, m = check(f"in flight, frame {k}", a, ents, 1, VIEWPORTS[1], VISIBLE, now, before, prev)
        assert (m == rr.NO_HISTORY).all() == (k == 0)
        before = now
    a.close()
    one, two = run_in_flight(app_mod, 1), run_in_flight(app_mod, 2)
    for k in range(4):
        assert np.array_equal(one[k][0], two[k][0]) and np.array_equal(one[k][1], two[k][1]), k
    assert (one[0][1] == rr.NO_HISTORY).all() and (one[3][1] == 0).any()


def test_multi_device_viewports_refuse_history_reprojection(app_mod, capfd):
    a, ents = make_app(app_mod, {1: VIEWPORTS[1]})
    assert a.set_history_reprojection(1, True)
    a.draw_frame()
    assert a.read_reprojection(1, *VIEWPORTS[1]) is not None
    capfd.readouterr()
    a.set_device_count(2, [0, 0])  # turns it off, and says so
    assert "history reprojection" in capfd.readouterr().err
    a.draw_frame()
    assert a.read_reprojection(1, *VIEWPORTS[1]) is None
    assert not a.set_history_reprojection(1, True)  # refused, with a log line
    assert "history reprojection" in capfd.readouterr().err
    a.draw_frame()
    assert a.read_reprojection(1, *VIEWPORTS[1]) is None and a.reprojection_textures(1) is None
    a.close()
