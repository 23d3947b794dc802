"""Device poses through the engine API on the GPU: a scene animated by ECS::AnimationSystem renders the same pixels
with Renderer::SetDevicePoseEnabled on as with the CPU system and the uploaded palette, without a host palette upload
per frame; with frames in flight; and as row bands of a group."""
import numpy as np
import pytest

import anim_cases
import anim_ref
from trident_raster import abi, app, scenes

pytestmark = pytest.mark.gpu

W, H = 160, 120
IDENT = np.eye(4, dtype=np.float32).reshape(16)


def _skinned_cube():
    """The primitive cube with every vertex on one of three bones by height."""
    v, i = scenes.cube_mesh()[:2]
    v = v.copy()
    y = v["position"][:, 1]
    v["bone_indices"][:, 0] = np.where(y > 0, 2, 1)
    v["bone_weights"][:] = 0.0
    v["bone_weights"][:, 0] = 1.0
    return v, i


def _scene(device_pose, frames_in_flight=1, devices=None):
    rig = next(r for r in anim_ref.kernel_rigs() if r.name == "chain3")
    anim_cases.cpu_asset(rig)
    a = app.TridentApp()
    if devices:
        a.set_device_count(len(devices), devices)
    a.set_frames_in_flight(frames_in_flight)
    a.set_camera("editor", (0.0, 0.5, 6.0))
    a.set_viewport(1, W, H)
    a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=4.0)
    mesh = a.append_mesh(*_skinned_cube())
    ents = [a.add_mesh_entity("none", mesh, position=(x, 0.0, 0.0), rotation=(20.0, 30.0, 0.0)) for x in (-2.0, 0.0, 2.0)]
    # two entities play the clip at different times (rotations held, translation and scale interpolating: the device
    # pose equals the CPU pose bit for bit); the third carries matrices written by other code (the uploaded prefix)
    a.set_entity_animation(ents[0], "test:chain3", "test:chain3", "hold", time=0.65, speed=1.0)
    a.set_entity_animation(ents[1], "test:chain3", "test:chain3", "hold", time=0.05, speed=2.0)
    a.set_device_pose(device_pose)
    return a, ents


def _frames(a, ents, n, dt=0.03125):
    host = np.tile(IDENT, (3, 1))
    host[2, 12] = 0.5
    out = []
    for _ in range(n):
        a.update_animation(dt)
        a.set_entity_bones(ents[2], host)
        a.draw_frame()
        a.finish_frame()
        out.append(a.read_pixels(1, W, H))
    return out


def test_device_mode_renders_the_cpu_path_frames_without_palette_uploads():
    cpu, ce = _scene(False)
    dev, de = _scene(True)
    fc, fd = _frames(cpu, ce, 4), _frames(dev, de, 4)
    for k, ((pc, zc), (pd, zd)) in enumerate(zip(fc, fd)):
        assert np.array_equal(zc, zd) and np.array_equal(pc, pd), f"frame {k}"
    assert not np.array_equal(fc[0][0], fc[3][0])  # the animation moves the picture
    # the skinned cubes are on screen: a unit cube 6 away is about 24 pixels across at this size, and there are three
    assert (fc[0][1] != 1.0).sum() > 24 * 24
    assert cpu.bone_palette_uploads() == 4  # a new palette every frame
    assert dev.bone_palette_uploads() == 1  # the static prefix once
    # host code that reads the pose still gets it
    t = dev.entity_animation_state(de[0])[0]
    h, clips = anim_cases.cpu_asset(next(r for r in anim_ref.kernel_rigs() if r.name == "chain3"))
    assert np.array_equal(dev.entity_pose(de[0]), app.anim_evaluate(h, clips[0], t))
    assert np.array_equal(cpu.entity_pose(ce[0]), dev.entity_pose(de[0]))
    # switching back uploads again and renders the same
    dev.set_device_pose(False)
    cpu_again = _frames(dev, de, 1)[0]
    want = _frames(cpu, ce, 1)[0]
    assert np.array_equal(cpu_again[0], want[0]) and dev.bone_palette_uploads() == 2
    cpu.close()
    dev.close()


def test_device_mode_with_frames_in_flight_and_row_bands():
    ref, re_ = _scene(False)
    want = _frames(ref, re_, 5)[-1]
    ring, ee = _scene(True, frames_in_flight=3)
    host = np.tile(IDENT, (3, 1))
    host[2, 12] = 0.5
    for _ in range(5):  # no wait between frames: each ring target is posed for its own frame
        ring.update_animation(0.03125)
        ring.set_entity_bones(ee[2], host)
        ring.draw_frame()
    ring.finish_frame()
    got = ring.read_pixels(1, W, H)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    bands, be = _scene(True, devices=[0, 0])  # a group of two bands: tri_group_pose_palette
    got = _frames(bands, be, 5)[-1]
    assert np.array_equal(got[1], want[1])
    assert int(np.abs(got[0].astype(np.int16) - want[0].astype(np.int16)).max()) <= 1
    for a in (ref, ring, bands):
        a.close()


def test_assets_registered_after_first_use_reach_the_device():
    """A clip appended, and a skeleton replaced, after the device already holds the asset: the next frame poses from
    what the service holds now, as the CPU path does."""
    lb = np.stack([anim_ref.compose([0.0, 0.2 * (b > 0), 0.0], [1, 0, 0, 0], [1, 1, 1]) for b in range(3)]).astype(np.float32)
    ib = np.tile(IDENT, (3, 1))
    frames = {}
    for mode in (False, True):
        h = app.anim_register("test:shim_late", [-1, 0, 1], lb, ib)
        a = app.TridentApp()
        a.set_camera("editor", (0.0, 0.5, 6.0))
        a.set_viewport(1, W, H)
        a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=4.0)
        e = a.add_mesh_entity("none", a.append_mesh(*_skinned_cube()), rotation=(20.0, 30.0, 0.0))
        a.set_entity_animation(e, "test:shim_late", "test:shim_late", "late", time=0.0, playing=False)
        a.set_device_pose(mode)
        out = []

        def frame():
            a.update_animation(0.0)
            a.draw_frame()
            a.finish_frame()
            out.append(a.read_pixels(1, W, H))

        frame()  # no clip of that name yet: the bind pose; the device holds the asset now
        ch = np.zeros(1, abi.POSE_CHANNEL_DTYPE)
        ch[0] = (2, 0, 1, 0, 0, 0, 0, 0)
        app.anim_add_clip(h, "late", 1.0, ch, [0.0], [[0.5, 0.2, 0.0]], [], np.zeros((0, 4)))
        # (a clip name is looked up again when it changes, as in the reference: name another clip for one update)
        a.set_entity_animation(e, "test:shim_late", "test:shim_late", "another", time=0.0, playing=False)
        a.update_animation(0.0)
        a.set_entity_animation(e, "test:shim_late", "test:shim_late", "late", time=0.0, playing=False)
        frame()  # the appended clip plays
        moved = lb.copy()
        moved[1, 12] = -0.5
        app.anim_register("test:shim_late", [-1, 0, 1], moved, ib)  # the skeleton replaced under its id (no clips)
        frame()
        frames[mode] = out
        a.close()
    for k, ((pc, zc), (pd, zd)) in enumerate(zip(frames[False], frames[True])):
        assert np.array_equal(zc, zd) and np.array_equal(pc, pd), f"frame {k}"
    assert not np.array_equal(frames[True][0][1], frames[True][1][1])  # the clip moved the top of the cube
    assert not np.array_equal(frames[True][1][1], frames[True][2][1])  # so did the new skeleton


def test_an_imported_gltf_character_animates_on_either_path():
    """The fixture rig imported as a model: its meshes carry the skin's influences, its ids resolve to the file's
    skeleton and clips, and the device poses it as the CPU system does (a translation clip: no sin / acos)."""
    import os

    rig = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "anim", "rig.gltf")
    frames = {}
    for mode in (False, True):
        a = app.TridentApp()
        a.set_camera("editor", (0.0, 0.0, 5.0))
        a.set_viewport(1, W, H)
        a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=4.0)
        ents = a.import_model(rig)
        assert len(ents) == 2
        a.draw_frame()
        a.finish_frame()
        still = a.read_pixels(1, W, H)
        for e in ents:
            a.set_entity_animation(e, rig, rig, "Clip1", time=0.25, speed=1.0)
        a.set_device_pose(mode)
        out = [still]
        for _ in range(3):
            a.update_animation(0.125)
            a.draw_frame()
            a.finish_frame()
            out.append(a.read_pixels(1, W, H))
        assert a.entity_animation_state(ents[0])[2:] == (app.anim_load(rig), app.anim_load(rig), 1)
        assert a.bone_palette_uploads() == (0 if mode else 3)
        frames[mode] = out
        a.close()
    for k, ((pc, zc), (pd, zd)) in enumerate(zip(frames[False], frames[True])):
        assert np.array_equal(zc, zd) and np.array_equal(pc, pd), f"frame {k}"
    # the bar is on screen: 0.2 x 2.5 units 5 away is about 6 x 72 pixels at this size
    assert (frames[True][0][1] != 1.0).sum() > 200
    assert not np.array_equal(frames[True][0][1], frames[True][1][1])  # skinned: it is no rigid mesh any more
    assert not np.array_equal(frames[True][1][1], frames[True][3][1])  # and it moves with the clip
