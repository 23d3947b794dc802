"""The frame generator inside the shim: Renderer::LoadAiModel + ProcessAiFrame on the GPU. The C1 cube at 64 x 48, both
throttles 0, a seeded 4-channel container. Every GPU step is bounded: FinishAiInference has a deadline and returns
false on it."""
import numpy as np
import pytest
import torch

import framegen_ref
import tensor_ref

pytestmark = pytest.mark.gpu

W, H = 64, 48
DEADLINE_MS = 20000


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """{channels: (state_dict, container path)}."""
    root = tmp_path_factory.mktemp("framegen")
    out = {}
    for channels, seed in ((4, 4104), (6, 4106)):
        state = framegen_ref.make_state(channels, seed)
        path = root / f"gen{channels}.trifgen"
        path.write_bytes(framegen_ref.container_bytes(state, channels))
        out[channels] = (state, path)
    return out


def _cube_app(app_mod, model=None):
    from trident_raster import scenes

    a = app_mod.TridentApp()
    a.set_assets_dir(scenes.ASSETS_DIR)
    a.set_camera("editor", (0.0, 3.0, 8.0), (-8.0, 15.0, 0.0))
    a.add_mesh_entity("cube", position=(0.0, 3.0, 2.0), rotation=(0.0, 30.0, 0.0), scale=(3.0, 3.0, 3.0))  # ~900 pixels
    a.set_viewport(1, W, H)
    if model is not None:
        a.load_ai_model(model)
        assert a.ai_readback_enabled()
    assert a.set_ai_readback(True, 0, 0)  # both throttles 0
    return a


def _one_inference(a):
    """DrawFrame, FinishFrame (the capture resolves, the tensor is submitted), FinishAiInference: the frame that was
    read back, RGBA8 [H, W, 4]."""
    a.draw_frame()
    a.finish_frame()
    assert a.finish_ai_inference(DEADLINE_MS)
    return a.read_pixels(1, W, H, depth=False)[0]


def _reference(state, rgba):
    """(R32, R64, e_ref) of the network on the tensor of an RGBA8 frame."""
    x = tensor_ref.tensor_from_rgba(rgba)  # (what tensor_from_bgra gives for the B8G8R8A8 target)
    r32 = framegen_ref.forward(state, x, torch.float32)
    r64 = framegen_ref.forward(state, x, torch.float64)
    return r32, r64, float(np.abs(r32.astype(np.float64) - r64).max())


def test_renderer_generates_its_own_blend_frame(app_mod, models, oracle):
    from trident_raster import scenes

    state, path = models[4]
    a = _cube_app(app_mod, path)
    a.set_ai_blend_strength(0.6)
    assert a.ai_model_info() == (True, [1, -1, -1, 4], [1, -1, -1, 3])
    frame0 = _one_inference(a)
    assert a.ai_model_info() == (True, [1, H, W, 4], [1, H, W, 3])
    a.draw_frame()  # blends the generated frame
    stats = a.ai_debug_stats()
    assert stats["model_initialised"] == 1 and stats["completed_inference_count"] == 1 and stats["pending_job_count"] == 0
    assert stats["last_inference_ms"] > 0.0 and stats["average_inference_ms"] == stats["last_inference_ms"]
    assert stats["texture_ready"] == 1 and (stats["texture_width"], stats["texture_height"]) == (W, H)
    assert stats["blend_strength"] == np.float32(0.6)
    blended = a.read_pixels(1, W, H, depth=False)[0]
    blend = a.read_ai_blend_frame()
    assert blend is not None and blend.shape == (H, W, 4)
    # the blend frame: the reference network on the tensor of the frame that was read back, packed as the host path packs
    r32, _, _ = _reference(state, frame0)
    want = framegen_ref.pack_rgba8(r32)
    assert np.array_equal(blend[..., 3], want[..., 3])
    assert np.abs(blend.astype(np.int16) - want.astype(np.int16)).max() <= 1
    assert int(blend[..., :3].max()) - int(blend[..., :3].min()) > 50  # not a flat frame
    # the next rendered frame: the oracle's AI-blend render of the same inputs with that frame
    ubo, draws = a.frame_inputs(1)
    assert list(ubo.ai_blend_config) == [np.float32(0.6), np.float32(1 / W), np.float32(1 / H), 1.0]
    vb, ib, ranges = a.geometry()
    s = scenes.Scene("shim_framegen", W, H, vb, ib, ranges, draws, ubo, materials=[(m[0], m[1]) for m in a.materials()],
                     skybox=scenes.reference_skybox(), ai_frame=blend)
    oc, od, _ = oracle.render(s)
    assert (od != 0x3F800000).sum() > 200
    assert not np.array_equal(blended, frame0)
    diff = np.abs(blended.astype(np.int16) - oc[..., [2, 1, 0, 3]].astype(np.int16))
    assert int(diff.max()) <= 1, int(diff.max())
    a.close()  # (with the second job in flight: Shutdown waits)


def _cube_pixels(frame):
    """Pixels that are not the background's (the solid skybox): the cube was rendered."""
    return int(np.any(frame != frame[0, 0], axis=-1).sum())


@pytest.mark.parametrize("in_flight", [1, 2])
def test_resize_through_an_extent_the_network_cannot_take(app_mod, models, in_flight):
    """64 x 48 -> 66 x 50 (no multiple of 4: the generator refuses it) -> 64 x 48, with a blend frame present, as a
    dragged editor viewport does. The refused extent keeps the generator and the frame it made: the resized targets
    pack it again, every frame renders, and back on a good extent the loop goes on."""
    _, path = models[4]
    a = _cube_app(app_mod, path)
    a.set_frames_in_flight(in_flight)
    a.set_ai_blend_strength(0.6)
    _one_inference(a)
    a.draw_frame()
    a.finish_frame()
    assert a.finish_ai_inference(DEADLINE_MS)
    blend0 = a.read_ai_blend_frame()
    assert blend0 is not None and blend0.shape == (H, W, 4)
    done = a.ai_debug_stats()["completed_inference_count"]
    assert done == 2

    a.set_viewport(1, W + 2, H + 2)
    for _ in range(in_flight + 1):  # every ring target at the new extent, and its tensor offered to the generator
        a.draw_frame()
        a.finish_frame()
        assert a.finish_ai_inference(DEADLINE_MS)
    stats = a.ai_debug_stats()
    assert stats["model_initialised"] == 1 and stats["pending_job_count"] == 0
    assert stats["completed_inference_count"] == done  # 66 x 50 was refused ...
    assert stats["texture_ready"] == 1 and (stats["texture_width"], stats["texture_height"]) == (W, H)  # ... the frame stays
    assert _cube_pixels(a.read_pixels(1, W + 2, H + 2, depth=False)[0]) > 200
    kept = a.read_ai_blend_frame()
    assert kept is not None and np.array_equal(kept, blend0)
    assert list(a.frame_inputs(1)[0].ai_blend_config) == [np.float32(0.6), np.float32(1 / W), np.float32(1 / H), 1.0]

    a.set_viewport(1, W, H)
    for _ in range(in_flight + 1):
        a.draw_frame()
        a.finish_frame()
        assert a.finish_ai_inference(DEADLINE_MS)
        assert _cube_pixels(a.read_pixels(1, W, H, depth=False)[0]) > 200
    stats = a.ai_debug_stats()
    assert stats["completed_inference_count"] > done and stats["texture_ready"] == 1
    assert a.read_ai_blend_frame() is not None
    a.close()


def test_resize_while_a_job_is_in_flight_does_not_stall_or_drop_the_frame(app_mod, models):
    """A target made while the next job rewrites the generator's tensor renders without waiting for that job (with the
    blend, if the job has just finished; without it otherwise) and gets the next output."""
    _, path = models[4]
    a = _cube_app(app_mod, path)
    a.set_ai_blend_strength(0.6)
    _one_inference(a)
    a.draw_frame()
    a.finish_frame()  # the second job is submitted here and nobody waits for it
    a.set_viewport(1, W // 2, H // 2)
    a.draw_frame()
    assert _cube_pixels(a.read_pixels(1, W // 2, H // 2, depth=False)[0]) > 50
    assert a.finish_ai_inference(DEADLINE_MS)
    a.draw_frame()
    a.finish_frame()
    assert a.finish_ai_inference(DEADLINE_MS)
    a.draw_frame()
    blend = a.read_ai_blend_frame()
    assert blend is not None and blend.shape == (H // 2, W // 2, 4)
    assert _cube_pixels(a.read_pixels(1, W // 2, H // 2, depth=False)[0]) > 50
    a.close()


def test_a_refused_file_leaves_the_running_model_alone(app_mod, models, tmp_path):
    _, path = models[4]
    a = _cube_app(app_mod, path)
    _one_inference(a)
    a.draw_frame()
    a.finish_frame()  # a job in flight
    bad = tmp_path / "bad.trifgen"
    bad.write_bytes(path.read_bytes()[:200])
    with pytest.raises(app_mod.TriError):
        a.load_ai_model(bad)
    assert a.ai_model_info()[0] and a.ai_debug_stats()["pending_job_count"] == 1
    assert a.finish_ai_inference(DEADLINE_MS)
    a.draw_frame()
    stats = a.ai_debug_stats()
    assert stats["model_initialised"] == 1 and stats["completed_inference_count"] == 2 and stats["texture_ready"] == 1
    assert a.read_ai_blend_frame() is not None
    a.close()


def test_dataset_sample_pairs_input_and_output(app_mod, models, tmp_path):
    state, path = models[4]
    a = _cube_app(app_mod, path)
    a.set_dataset_capture(True, tmp_path / "cap", 1)
    frame0 = _one_inference(a)
    blend = a.read_ai_blend_frame()
    a.set_dataset_capture(False)  # flushes
    a.close()
    root = tmp_path / "cap"
    assert [p.name for p in (root / "inputs").iterdir()] == ["frame_000000.npy"]
    assert [p.name for p in (root / "metadata").iterdir()] == ["frame_000000.json"]
    assert [p.name for p in (root / "outputs").iterdir()] == ["ai_000000.npy"]
    x = tensor_ref.tensor_from_rgba(frame0)
    assert (root / "inputs/frame_000000.npy").read_bytes() == tensor_ref.npy_bytes(x, (1, H, W, 4))
    assert (root / "metadata/frame_000000.json").read_text() == tensor_ref.metadata_text(W, H, 4, (1, H, W, 4))
    out = np.load(root / "outputs/ai_000000.npy")
    assert out.shape == (1, H, W, 3) and out.dtype == np.float32
    # the normalised tensor: channels 0 and 2 swapped, within [0, 1] — the one whose packing is the device's blend frame,
    # and the reference network's output within the measured bound
    assert out.min() >= 0.0 and out.max() <= 1.0
    assert np.array_equal(framegen_ref.pack_rgba8(out[0][..., [2, 1, 0]]), blend)
    r32, r64, e_ref = _reference(state, frame0)
    err = float(np.abs(out[0][..., [2, 1, 0]].astype(np.float64) - r64).max())
    print(f"framegen shim {H}x{W}: e_ref {e_ref:.3e} gpu error {err:.3e} ratio {err / e_ref:.3f}")
    assert err <= framegen_ref.BOUND_M * e_ref, (err, e_ref)


def test_six_channel_model_submits_nothing(app_mod, models):
    """The readback tensor has 4 channels: the element count differs from the model's input, so the renderer warns and
    skips (Renderer.cpp:957-963), and the blend stays off."""
    _, path = models[6]
    a = _cube_app(app_mod, path)
    assert a.ai_model_info() == (True, [1, -1, -1, 6], [1, -1, -1, 3])
    for _ in range(2):
        a.draw_frame()
        a.finish_frame()
        assert a.finish_ai_inference(0)  # nothing in flight
    stats = a.ai_debug_stats()
    assert stats["model_initialised"] == 1 and stats["completed_inference_count"] == 0 and stats["pending_job_count"] == 0
    assert stats["texture_ready"] == 0 and (stats["texture_width"], stats["texture_height"]) == (0, 0)
    assert list(a.frame_inputs(1)[0].ai_blend_config) == [0.0, 0.0, 0.0, 0.0]
    assert a.read_ai_blend_frame() is None
    a.close()


def test_manual_path_still_works_with_a_model_loaded(app_mod, models):
    _, path = models[4]
    a = _cube_app(app_mod, path)
    before = _one_inference(a)  # the generator's own frame is the blend frame now
    assert a.read_ai_blend_frame() is not None
    rng = np.random.default_rng(9)
    out = rng.integers(0, 256, (H, W, 3)).astype(np.float32)  # a generator outside that answers in [0, 255]
    assert a.submit_ai_output(out, (-1, H, W, 3))
    a.set_ai_blend_strength(1.0)
    a.draw_frame()
    blended = a.read_pixels(1, W, H, depth=False)[0]
    want = tensor_ref.normalise_ai_output(out, 3)
    texels = np.round(want.reshape(H, W, 3) * np.float32(255)).astype(np.uint8)
    changed = np.any(blended != before, axis=-1)
    assert changed.sum() > 200
    assert np.array_equal(blended[changed][:, :3], texels[changed])  # at full strength a mesh pixel is its AI texel
    a.close()
