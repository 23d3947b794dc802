"""Temporal anti-aliasing through the engine API on the GPU: Renderer::SetTemporalAntiAliasingEnabled,
ReadViewportResolvedPixels, ReadViewportTaaMask, GetViewportResolvedTexture and the present over a flat-shaded sprite
whose slanted edge crosses the frame over a solid white skybox (a light of intensity 0: two colours, so "not constant"
means the silhouette), in two viewports, across a resize, with frames in flight, and refused on multi-device viewports.

Which jitter a frame was rendered under is read off its depth: the viewport's depth equals, bit for bit, the oracle's
depth of the frame's inputs under tri_taa_jitter(frameIndex, period). The resolved image is compared with
tests/taa_ref.py's restatement over the viewport's own colour, ids and depth (zero mismatches) and with the CPU truth,
the mean of an 8 x 8 sub-pixel grid of jittered oracle frames."""
import numpy as np
import pytest

import motion_ref as mr
import taa_ref as tr
from test_id_shim_gpu import NONE

pytestmark = pytest.mark.gpu
F = np.float32
SKY = np.full((6, 4, 4, 4), 255, np.uint8)  # a solid white cubemap: one background colour, far from the sprite's
SIZE = (64, 48)
PERIOD, ALPHA = 8, 0.1
NAMES = ("sprite",)


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


def make_app(app_mod, viewports=None):
    a = app_mod.TridentApp()
    a.set_camera("editor", (0.0, 1.0, 7.0), far=60.0)
    a.set_camera("runtime", (0.3, 1.2, 6.5), (0.0, 3.0, 0.0), far=60.0)
    for vp, (w, h) in (viewports or {1: SIZE}).items():
        a.set_viewport(vp, w, h)
    a.set_skybox(SKY)
    a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=0.0)  # ambient alone: the sprite is one colour
    ents = {"sprite": a.add_sprite_entity(position=(2.8, 1.0, 1.5), rotation=(0.0, 180.0, 20.0), scale=(5.0, 14.0, 1.0),
                                          tint=(0.9, 0.4, 0.2, 1.0))}
    return a, ents


def scene_of(a, vp, size):
    """The viewport's next frame, unjittered, as an oracle scene."""
    from trident_raster import scenes

    ubo, draws = a.frame_inputs(vp)
    vb, ib, ranges = a.geometry()
    return scenes.Scene(f"taa_shim_vp{vp}", size[0], size[1], vb, ib, ranges, draws, ubo,
                        materials=[(m[0], m[1]) for m in a.materials()], skybox=SKY)


def frame_of(a, ents, vp, size):
    """(ids, depth bits, colour B G R A) of the viewport's latest RAW frame."""
    w, h = size
    entity = a.read_entity_ids(vp, w, h)
    assert entity is not None  # the request turned the id output on
    ids = np.zeros((h, w), np.uint32)
    for d, n in enumerate(NAMES):
        ids[entity == ents[n]] = d + 1
    assert ((ids != 0) == (entity != NONE)).all()
    rgba, depth = a.read_pixels(vp, w, h)
    return ids, np.ascontiguousarray(depth).view(np.uint32), np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])


def resolved_of(a, vp, size):
    got = a.read_resolved(vp, *size)
    assert got is not None
    return np.ascontiguousarray(got[0][..., [2, 1, 0, 3]]), got[1]  # B G R A like the frames


def assert_jitter_index(oracle, scene, depth_bits, index, tag):
    """The frame was rendered under tri_taa_jitter(index, PERIOD) — and under no other of the period's offsets."""
    from trident_raster import raster

    same = [k for k in range(PERIOD)
            if np.array_equal(oracle.render(tr.jittered(scene, *raster.taa_jitter(k, PERIOD)))[1], depth_bits)]
    assert index % PERIOD in same, (tag, index, same)
    assert len(same) < PERIOD, tag  # (the silhouette moves under the jitter: the depth tells offsets apart)


def frame_of_raw(a, vp, size):
    rgba, _ = a.read_pixels(vp, *size)
    return np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])


def run(oracle, a, ents, vps, frames, state, move=None, check_index=True):
    """`frames` DrawFrames; after each, every viewport in vps ({vp: size}) against the restatement, chained through
    state[vp] = {"index", "prev", "before"}. Returns {vp: [(resolved, mask)]}."""
    from trident_raster import raster

    outs = {vp: [] for vp in vps}
    for _ in range(frames):
        if move:
            move()
        now = {vp: scene_of(a, vp, size) for vp, size in vps.items()}
        a.draw_frame()
        for vp, size in vps.items():
            st = state.setdefault(vp, {"index": 0, "prev": None, "before": None})
            s = now[vp]
            ids, dep, col = frame_of(a, ents, vp, size)
            if check_index:
                assert_jitter_index(oracle, s, dep, st["index"], f"viewport {vp} frame {st['index']}")
            jx, jy = raster.taa_jitter(st["index"], PERIOD)
            cur = tr.jittered(s, jx, jy)
            hist = None
            if st["before"] is not None:  # the previous view and UNJITTERED projection, under this frame's jitter
                hist = tr.contract_history(s, jx, jy, *mr.camera_of(st["before"].ubo), mr.models_of(st["before"].draws))
            table = raster.motion_matrices(cur.ubo, cur.draws, hist)
            acc, want, want_m = tr.restate(table, ids, dep, col, st["prev"], size[0], size[1], ALPHA)
            got, got_m = resolved_of(a, vp, size)
            bad_m, bad_c = int((got_m != want_m).sum()), int((got != want).any(axis=-1).sum())
            print(f"SHIM TAA viewport {vp} frame {st['index']}: valid {int(((want_m & 15) == 0).sum())}, none "
                  f"{int((want_m == 1).sum())}, mask mismatches {bad_m}, resolved mismatches {bad_c}")
            assert bad_m == 0 and bad_c == 0, (vp, st["index"])
            st.update(index=st["index"] + 1, prev=(acc, ids), before=s)
            outs[vp].append((got, got_m))
    return outs


def test_a_static_silhouette_converges_and_flat_pixels_stay_exact(app_mod, oracle):
    from trident_raster import abi

    a, ents = make_app(app_mod)
    s = scene_of(a, 1, SIZE)
    a.draw_frame()
    assert a.read_resolved(1, *SIZE) is None and a.resolved_texture(1) is None and not a.is_temporal_anti_aliasing(1)
    raw = frame_of_raw(a, 1, SIZE)
    grid = [(i + 0.5) / 8.0 - 0.5 for i in range(8)]
    truth = np.mean([oracle.render(tr.jittered(s, jx, jy))[0].astype(np.float64) for jy in grid for jx in grid], axis=0)
    edge, flat = tr.silhouette(raw), tr.flat5(raw)

    def err(img):
        return float(np.abs(img[..., :3].astype(np.float64) - truth[..., :3])[edge].mean())

    e0 = err(raw)
    assert edge.sum() >= 48 and e0 > 4.0 and flat.sum() > 0.5 * flat.size
    assert not a.set_temporal_anti_aliasing(1, True, 0.0) and not a.set_temporal_anti_aliasing(1, True, 1.5)  # refused
    assert not a.set_temporal_anti_aliasing(1, True, 0.1, 65) and not a.is_temporal_anti_aliasing(1)
    assert a.set_temporal_anti_aliasing(1, True, ALPHA, PERIOD) and a.is_temporal_anti_aliasing(1)
    errs = []
    for n in range(40):
        a.draw_frame()
        if n == 0 or n >= 32:
            got, mask = resolved_of(a, 1, SIZE)
            assert (mask == tr.NO_HISTORY).all() if n == 0 else (mask == 0).all(), n
            assert np.array_equal(got[flat], raw[flat]), n
            if n >= 32:
                errs.append(err(got))
    print(f"SHIM TAA quality: {int(edge.sum())} silhouette pixels, raw error E0 {e0:.2f} LSB; resolved, frames 32..39: "
          + " ".join(f"{e:.2f}" for e in errs) + f"; worst ratio {max(errs) / e0:.3f}")
    assert max(errs) <= 0.5 * e0
    img = a.resolved_texture(1)
    assert (img.width, img.height, img.pitch_bytes, img.format) == (*SIZE, SIZE[0] * 4, abi.TRI_FORMAT_B8G8R8A8_UNORM) and img.device_ptr
    # the viewport's own readers keep the raw, jittered frame: it differs from the unjittered one on the silhouette only
    jit = frame_of_raw(a, 1, SIZE)
    assert np.array_equal(jit[flat], raw[flat]) and not np.array_equal(jit, raw)
    a.close()


def test_off_is_bit_identical_to_never_on(app_mod):
    def frames(switch):
        a, ents = make_app(app_mod)
        out = []
        for k in range(5):
            if switch and k == 1:
                assert a.set_temporal_anti_aliasing(1, True)
            if switch and k == 3:
                assert a.set_temporal_anti_aliasing(1, False)
            a.set_camera("editor", (0.1 * k, 1.0, 7.0 - 0.1 * k), (0.0, 1.5 * k, 0.0), far=60.0)
            a.draw_frame()
            rgba, depth = a.read_pixels(1, *SIZE)
            out.append((rgba, np.ascontiguousarray(depth).view(np.uint32), a.read_resolved(1, *SIZE)))
        a.close()
        return out

    never, switched = frames(False), frames(True)
    for k in (0, 3, 4):  # off: the frame is the one a renderer that never had it on renders
        assert np.array_equal(never[k][0], switched[k][0]) and np.array_equal(never[k][1], switched[k][1]), k
        assert switched[k][2] is None
    for k in (1, 2):  # on: resolved, and (frame index 1: a quarter of a pixel to the left) rendered under the jitter
        assert switched[k][2] is not None, k
    assert not np.array_equal(never[2][1], switched[2][1])


def test_two_viewports_have_their_own_history_and_frame_index_and_a_resize_restarts(app_mod, oracle):
    vps = {1: SIZE, 2: (58, 40)}
    a, ents = make_app(app_mod, vps)
    k = [0]

    def move():
        k[0] += 1
        a.set_camera("editor", (0.05 * k[0], 1.0, 7.0 - 0.05 * k[0]), (0.0, 0.5 * k[0], 0.0), far=60.0)
        a.set_camera("runtime", (0.3 - 0.04 * k[0], 1.2, 6.5), (0.0, 3.0 - 0.4 * k[0], 0.0), far=60.0)

    state = {}
    assert a.set_temporal_anti_aliasing(1, True, ALPHA, PERIOD)
    outs = run(oracle, a, ents, {1: SIZE}, 3, state, move)  # viewport 1 alone: frames 0, 1, 2
    assert (outs[1][0][1] == tr.NO_HISTORY).all() and all(((m & 15) == 0).any() for _, m in outs[1][1:])
    assert a.read_resolved(2, *vps[2]) is None
    assert a.set_temporal_anti_aliasing(2, True, ALPHA, PERIOD)
    outs = run(oracle, a, ents, vps, 3, state, move)  # viewport 1 at frames 3..5, viewport 2 at 0..2
    assert (outs[2][0][1] == tr.NO_HISTORY).all() and not (outs[1][0][1] == tr.NO_HISTORY).any()
    assert state[1]["index"] == 6 and state[2]["index"] == 3
    # a resize: a new object and the count from 0; the other viewport keeps both
    a.set_viewport(1, 80, 50)
    vps[1] = (80, 50)
    state[1] = {"index": 0, "prev": None, "before": None}
    outs = run(oracle, a, ents, vps, 2, state, move)
    assert (outs[1][0][1] == tr.NO_HISTORY).all() and ((outs[1][1][1] & 15) == 0).any()
    assert not (outs[2][0][1] == tr.NO_HISTORY).any()
    # off: the readers answer no more; on again: no history once, the count from 0
    assert a.set_temporal_anti_aliasing(1, False)
    a.draw_frame()
    assert a.read_resolved(1, 80, 50) is None and a.resolved_texture(1) is None
    assert a.set_temporal_anti_aliasing(1, True, ALPHA, PERIOD)
    state[1] = {"index": 0, "prev": None, "before": None}
    outs = run(oracle, a, ents, {1: (80, 50)}, 2, state, move)
    assert (outs[1][0][1] == tr.NO_HISTORY).all() and ((outs[1][1][1] & 15) == 0).any()
    assert a.read_resolved(9, 4, 4) is None  # no such viewport
    a.close()


def run_in_flight(app_mod, oracle, n):
    a, ents = make_app(app_mod)
    a.set_frames_in_flight(n)
    assert a.set_temporal_anti_aliasing(1, True, ALPHA, PERIOD)
    k = [0]

    def move():
        k[0] += 1
        a.set_camera("editor", (0.05 * k[0], 1.0, 7.0 - 0.05 * k[0]), (0.0, 0.5 * k[0], 0.0), far=60.0)

    out = run(oracle, a, ents, {1: SIZE}, 5, {}, move, check_index=(n == 2))[1]
    a.close()
    return out


def test_two_frames_in_flight_equal_one(app_mod, oracle):
    """The history is the viewport's, not the ring target's: frame k accumulates over frame k - 1, which the other target
    rendered."""
    one, two = run_in_flight(app_mod, oracle, 1), run_in_flight(app_mod, oracle, 2)
    for k in range(5):
        assert np.array_equal(one[k][0], two[k][0]) and np.array_equal(one[k][1], two[k][1]), k
    assert (one[0][1] == tr.NO_HISTORY).all() and ((one[4][1] & 15) == 0).any()


def test_the_present_shows_the_resolved_image(app_mod):
    a, ents = make_app(app_mod)
    a.set_present_extent(*SIZE)  # the blit at the frame's own extent is a copy
    a.draw_frame()
    assert np.array_equal(a.read_present(*SIZE), a.read_pixels(1, *SIZE)[0])  # off: the raw frame
    assert a.set_temporal_anti_aliasing(1, True, ALPHA, PERIOD)
    for k in range(4):
        a.draw_frame()
        present = a.read_present(*SIZE)
        resolved = a.read_resolved(1, *SIZE)[0]
        assert np.array_equal(present, resolved), k
    assert not np.array_equal(present, a.read_pixels(1, *SIZE)[0])  # (the raw frame is another image by now)
    a.set_present_extent(2 * SIZE[0], 2 * SIZE[1])
    a.draw_frame()
    assert a.read_present(2 * SIZE[0], 2 * SIZE[1]).shape == (2 * SIZE[1], 2 * SIZE[0], 4)
    assert a.set_temporal_anti_aliasing(1, False)
    a.set_present_extent(*SIZE)
    a.draw_frame()
    assert np.array_equal(a.read_present(*SIZE), a.read_pixels(1, *SIZE)[0])
    a.close()


def test_multi_device_viewports_refuse_temporal_anti_aliasing(app_mod, capfd):
    a, ents = make_app(app_mod)
    assert a.set_temporal_anti_aliasing(1, True)
    a.draw_frame()
    assert a.read_resolved(1, *SIZE) is not None
    capfd.readouterr()
    a.set_device_count(2, [0, 0])  # turns it off, and says so
    assert "temporal anti-aliasing" in capfd.readouterr().err
    assert not a.is_temporal_anti_aliasing(1)
    a.draw_frame()
    assert a.read_resolved(1, *SIZE) is None
    assert not a.set_temporal_anti_aliasing(1, True)  # refused, with a log line
    assert "temporal anti-aliasing" in capfd.readouterr().err
    a.draw_frame()
    assert a.read_resolved(1, *SIZE) is None and a.resolved_texture(1) is None
    a.close()
