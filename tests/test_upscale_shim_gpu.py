"""Temporal upscaling through the engine API on the GPU: Renderer::SetTemporalUpscalingEnabled,
ReadViewportUpscaledPixels, ReadViewportUpscaleMask, GetViewportUpscaledTexture and the present, over
test_taa_shim_gpu.py's scene: a flat-shaded sprite whose slanted edge crosses the frame over a solid white skybox (two
colours, so "not constant" means the silhouette), on a 64 x 48 viewport rendered at 32 x 24.

The upscaled image is compared with tests/upscale_ref.py's restatement over the viewport's own raw colour, ids and depth
(zero mismatches) and with the CPU truth, the mean of an 8 x 8 sub-pixel grid of oracle frames at 64 x 48."""
import numpy as np
import pytest

import motion_ref as mr
import taa_ref as tr
import upscale_ref as ur

pytestmark = pytest.mark.gpu
F = np.float32
NONE = 0xFFFFFFFF  # ReadViewportEntityIds' background
SKY = np.full((6, 4, 4, 4), 255, np.uint8)  # a solid white cubemap: one background colour, far from the sprite's
SIZE, RENDER = (64, 48), (32, 24)
ALPHA = 0.1
NAMES = ("sprite",)


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


def make_app(app_mod, size=SIZE):
    a = app_mod.TridentApp()
    a.set_camera("editor", (0.0, 1.0, 7.0), far=60.0)
    a.set_camera("runtime", (0.3, 1.2, 6.5), (0.0, 3.0, 0.0), far=60.0)
    a.set_viewport(1, *size)
    a.set_skybox(SKY)
    a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=0.0)  # ambient alone: the sprite is one colour
    ents = {"sprite": a.add_sprite_entity(position=(2.8, 1.0, 1.5), rotation=(0.0, 180.0, 20.0), scale=(5.0, 14.0, 1.0),
                                          tint=(0.9, 0.4, 0.2, 1.0))}
    return a, ents


def scene_of(a, vp, size):
    """The viewport's next frame, unjittered, as an oracle scene at `size`."""
    from trident_raster import scenes

    ubo, draws = a.frame_inputs(vp)
    vb, ib, ranges = a.geometry()
    return scenes.Scene(f"upscale_shim_vp{vp}", size[0], size[1], vb, ib, ranges, draws, ubo,
                        materials=[(m[0], m[1]) for m in a.materials()], skybox=SKY)


def raw_of(a, vp, size):
    """The viewport's latest RAW colour, B G R A, at the extent its context has."""
    return np.ascontiguousarray(a.read_pixels(vp, *size)[0][..., [2, 1, 0, 3]])


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


def upscaled_of(a, vp, size):
    got = a.read_upscaled(vp, *size)
    assert got is not None
    return np.ascontiguousarray(got[0][..., [2, 1, 0, 3]]), got[1]  # B G R A like the frames


def run(a, ents, size, render, frames, state, move=None):
    """`frames` DrawFrames; after each, viewport 1 against the restatement, chained through state = {"index", "prev",
    "before"}. Returns [(upscaled, mask)]."""
    from trident_raster import raster

    period = raster.upscale_jitter_period(*render, *size)
    outs = []
    for _ in range(frames):
        if move:
            move()
        s = scene_of(a, 1, render)  # the viewport's matrices, rendered at the render extent
        a.draw_frame()
        img = a.viewport_texture(1)
        assert (img.width, img.height) == render
        ids, dep, col = frame_of(a, ents, 1, render)
        jx, jy = raster.taa_jitter(state["index"], period)
        cur = tr.jittered(s, jx, jy)
        hist = None
        if state["before"] is not None:  # the previous view and UNJITTERED projection, under this frame's jitter
            hist = tr.contract_history(s, jx, jy, *mr.camera_of(state["before"].ubo), mr.models_of(state["before"].draws))
        table = raster.motion_matrices(cur.ubo, cur.draws, hist)
        acc, want, want_m = ur.restate(table, ids, dep, col, state["prev"], size[0], size[1], (jx, jy), ALPHA)
        got, got_m = upscaled_of(a, 1, size)
        bad_m, bad_c = int((got_m != want_m).sum()), int((got != want).any(axis=-1).sum())
        print(f"SHIM UPSCALE {render} -> {size} frame {state['index']}: valid {int(((want_m & 15) == 0).sum())}, none "
              f"{int((want_m == 1).sum())}, mask mismatches {bad_m}, upscaled mismatches {bad_c}")
        assert bad_m == 0 and bad_c == 0, state["index"]
        state.update(index=state["index"] + 1, prev=(acc, ids), before=s)
        outs.append((got, got_m))
    return outs


def fresh():
    return {"index": 0, "prev": None, "before": None}


def test_a_static_silhouette_is_no_worse_than_the_native_frame(app_mod, oracle, capfd):
    """E_up <= E_native in each of the last 32 of 128 DrawFrames, against the shim's own unjittered 64 x 48 render.
    DESIGN 5q records the printed values."""
    from trident_raster import abi

    a, ents = make_app(app_mod)
    s = scene_of(a, 1, SIZE)
    a.draw_frame()
    assert a.read_upscaled(1, *SIZE) is None and a.upscaled_texture(1) is None and not a.is_temporal_upscaling(1)
    native = raw_of(a, 1, SIZE)
    grid = [(i + 0.5) / 8.0 - 0.5 for i in range(8)]
    truth = np.mean([oracle.render(tr.jittered(s, jx, jy))[0].astype(np.float64) for jy in grid for jx in grid], axis=0)
    edge = tr.silhouette(native)

    def err(img):
        return float(np.abs(img[..., :3].astype(np.float64) - truth[..., :3])[edge].mean())

    e_native = err(native)
    assert edge.sum() >= 48 and e_native > 4.0
    capfd.readouterr()
    for scale, alpha in ((0.2, ALPHA), (1.5, ALPHA), (float("nan"), ALPHA), (1.0 / 3.0, ALPHA), (0.5, 0.0), (0.5, 1.5)):
        assert not a.set_temporal_upscaling(1, True, scale, alpha), (scale, alpha)  # (1 / 3: 21 x 16, and 3 x 21 < 64)
        assert "temporal upscaling" in capfd.readouterr().err and not a.is_temporal_upscaling(1)
    assert a.set_temporal_upscaling(1, True, 0.5, ALPHA) and a.is_temporal_upscaling(1)
    errs = []
    for n in range(128):
        a.draw_frame()
        if n == 0:
            got, mask = upscaled_of(a, 1, SIZE)
            assert (mask == ur.NO_HISTORY).all()
            img = a.viewport_texture(1)
            assert (img.width, img.height) == RENDER  # ReadViewportPixels and GetViewportTexture: the raw 32 x 24 frame
            assert a.read_pixels(1, *RENDER)[0].shape == (RENDER[1], RENDER[0], 4)
        if n >= 96:
            got, mask = upscaled_of(a, 1, SIZE)
            assert not (mask & (ur.ID | ur.OUTSIDE | ur.NO_PROJ | ur.NO_HISTORY)).any(), n
            errs.append(err(got))
    e_near = err(ur.nearest(raw_of(a, 1, RENDER), *SIZE))
    print(f"SHIM UPSCALE quality: {int(edge.sum())} silhouette pixels, E_native {e_native:.2f} LSB, nearest-enlarged jittered raw "
          f"frame {e_near:.2f} LSB; E_up over frames 96..127: min {min(errs):.2f} mean {np.mean(errs):.2f} max {max(errs):.2f}; "
          f"worst ratio to native {max(errs) / e_native:.3f}")
    for n, e in enumerate(errs):
        assert e <= e_native, (96 + n, e, e_native)
    img = a.upscaled_texture(1)
    assert (img.width, img.height, img.pitch_bytes, img.format) == (*SIZE, SIZE[0] * 4, abi.TRI_FORMAT_B8G8R8A8_UNORM) and img.device_ptr
    a.close()


def test_the_present_shows_the_upscaled_image(app_mod):
    a, ents = make_app(app_mod)
    a.set_present_extent(*SIZE)  # the blit at the upscaled image's own extent is a copy
    a.draw_frame()
    assert np.array_equal(a.read_present(*SIZE), a.read_pixels(1, *SIZE)[0])  # off: the raw frame
    assert a.set_temporal_upscaling(1, True, 0.5, ALPHA)
    for k in range(4):
        a.draw_frame()
        assert np.array_equal(a.read_present(*SIZE), a.read_upscaled(1, *SIZE)[0]), k
    assert a.set_temporal_upscaling(1, False)
    a.draw_frame()
    assert a.read_upscaled(1, *SIZE) is None and a.upscaled_texture(1) is None
    assert np.array_equal(a.read_present(*SIZE), a.read_pixels(1, *SIZE)[0])
    a.close()


def test_off_is_bit_identical_to_never_on(app_mod):
    def frames(switch):
        a, ents = make_app(app_mod)
        out = []
        for k in range(5):
            if switch and k == 1:
                assert a.set_temporal_upscaling(1, True)
            if switch and k == 3:
                assert a.set_temporal_upscaling(1, False)
            a.set_camera("editor", (0.1 * k, 1.0, 7.0 - 0.1 * k), (0.0, 1.5 * k, 0.0), far=60.0)
            a.draw_frame()
            img = a.viewport_texture(1)
            size = (img.width, img.height)
            rgba, depth = a.read_pixels(1, *size)
            out.append((size, rgba, np.ascontiguousarray(depth).view(np.uint32), a.read_upscaled(1, *SIZE)))
        a.close()
        return out

    never, switched = frames(False), frames(True)
    for k in (0, 3, 4):  # off: the frame is the one a renderer that never had it on renders
        assert switched[k][0] == SIZE and switched[k][3] is None
        assert np.array_equal(never[k][1], switched[k][1]) and np.array_equal(never[k][2], switched[k][2]), k
    for k in (1, 2):  # on: rendered at half the size, and upscaled
        assert switched[k][0] == RENDER and switched[k][3] is not None, k


def test_a_moving_camera_a_resize_and_a_scale_change(app_mod):
    """Zero mismatches against the restatement under a moving camera; a resize and another scale make a new object: no
    history once, the jitter index from 0."""
    a, ents = make_app(app_mod)
    k = [0]

    def move():
        k[0] += 1
        a.set_camera("editor", (0.05 * k[0], 1.0, 7.0 - 0.05 * k[0]), (0.0, 0.5 * k[0], 0.0), far=60.0)

    assert a.set_temporal_upscaling(1, True, 0.5, ALPHA)
    outs = run(a, ents, SIZE, RENDER, 5, fresh(), move)
    assert (outs[0][1] == ur.NO_HISTORY).all() and all(((m & 15) == 0).any() for _, m in outs[1:])
    a.set_viewport(1, 80, 50)  # a resize
    outs = run(a, ents, (80, 50), (40, 25), 2, fresh(), move)
    assert (outs[0][1] == ur.NO_HISTORY).all() and ((outs[1][1] & 15) == 0).any()
    assert a.set_temporal_upscaling(1, True, 0.75, ALPHA)  # another scale
    outs = run(a, ents, (80, 50), (60, 38), 2, fresh(), move)
    assert (outs[0][1] == ur.NO_HISTORY).all() and ((outs[1][1] & 15) == 0).any()
    assert a.read_upscaled(9, 4, 4) is None  # no such viewport
    a.close()


def test_exclusive_with_temporal_anti_aliasing_and_refused_on_several_devices(app_mod, capfd):
    a, ents = make_app(app_mod)
    assert a.set_temporal_anti_aliasing(1, True)
    capfd.readouterr()
    assert not a.set_temporal_upscaling(1, True) and "temporal upscaling" in capfd.readouterr().err  # the later request
    assert a.is_temporal_anti_aliasing(1) and not a.is_temporal_upscaling(1)
    assert a.set_temporal_anti_aliasing(1, False) and a.set_temporal_upscaling(1, True)
    assert not a.set_temporal_anti_aliasing(1, True) and "temporal anti-aliasing" in capfd.readouterr().err
    assert a.is_temporal_upscaling(1) and not a.is_temporal_anti_aliasing(1)
    a.draw_frame()
    assert a.read_upscaled(1, *SIZE) is not None and a.read_resolved(1, *SIZE) is None
    a.set_device_count(2, [0, 0])  # turns it off, and says so
    assert "temporal upscaling" in capfd.readouterr().err
    assert not a.is_temporal_upscaling(1)
    a.draw_frame()
    assert a.read_upscaled(1, *SIZE) is None
    assert not a.set_temporal_upscaling(1, True)  # refused, with a log line
    assert "temporal upscaling" in capfd.readouterr().err
    a.draw_frame()
    assert a.read_upscaled(1, *SIZE) is None and a.upscaled_texture(1) is None
    a.close()


def test_the_ai_tensor_keeps_the_raw_frame_picking_keeps_viewport_pixels_and_recording_is_refused(app_mod, capfd, tmp_path):
    a, ents = make_app(app_mod)
    a.set_present_extent(*SIZE)  # the readback wants the present extent to be the viewport's SIZE, whatever it renders at
    assert a.set_ai_readback(True, 0, 0)
    assert a.set_temporal_upscaling(1, True, 0.5, ALPHA)
    a.draw_frame()
    a.finish_frame()
    tensor = a.acquire_frame()
    assert tensor is not None and tensor.shape == (RENDER[1], RENDER[0], 4)  # the raw frame at the render extent
    raw = a.read_pixels(1, *RENDER)[0]
    assert np.array_equal(tensor, raw.astype(F) * (F(1.0) / F(255.0)))
    dev = a.readback_device_tensor()
    assert dev is not None and dev[1:] == RENDER
    # picking takes viewport pixels: the render pixel that holds the viewport pixel's centre answers
    entity = a.read_entity_ids(1, *RENDER)
    inside = ~tr.window(entity != ents["sprite"], np.logical_or)
    outside = ~tr.window(entity != NONE, np.logical_or)
    assert inside.any() and outside.any()
    (yi, xi), (yo, xo) = np.argwhere(inside)[-1], np.argwhere(outside)[0]
    for dx, dy in ((0, 0), (1, 1)):
        hit = a.pick_entity(1, 2 * xi + dx, 2 * yi + dy)
        assert hit is not None and hit[0] == ents["sprite"]
        assert a.pick_entity(1, 2 * xo + dx, 2 * yo + dy) is None
    corner = a.pick_entity(1, SIZE[0] - 1, SIZE[1] - 1)  # beyond the render extent, inside the viewport
    assert (corner is None) == (entity[-1, -1] == NONE) and (corner is None or corner[0] == entity[-1, -1])
    assert a.pick_entity(1, SIZE[0], 0) is None and a.pick_entity(1, -1, 0) is None
    assert a.pick_entities_in_rect(1, 0, 0, SIZE[0] - 1, SIZE[1] - 1) == [ents["sprite"]]
    assert a.pick_entities_in_rect(1, 2 * xo, 2 * yo, 2 * xo + 1, 2 * yo + 1) == []
    # a recording session has one extent, the viewport's size: the two switches refuse each other, with one log line
    path = str(tmp_path / "upscaled.y4m")
    capfd.readouterr()
    assert not a.set_recording(True, 1, *SIZE, path)[0]
    assert "temporal upscaling" in capfd.readouterr().err and not a.recording_state()[0] and a.is_temporal_upscaling(1)
    assert a.set_temporal_upscaling(1, False)
    assert a.set_recording(True, 1, *SIZE, path)[0]
    assert not a.set_temporal_upscaling(1, True) and "is being recorded" in capfd.readouterr().err
    assert not a.is_temporal_upscaling(1)
    a.draw_frame()
    a.finish_frame()
    assert a.recording_state() == (True, 1)  # the full-size frame was recorded
    assert a.viewport_texture(1).width == SIZE[0]
    assert a.set_recording(False)[0]
    assert a.set_temporal_upscaling(1, True)  # ... and once the session is over the switch is taken again
    a.close()
