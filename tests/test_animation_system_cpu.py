"""ECS::AnimationSystem and the renderer's host-side palette layout with device poses on, without a GPU: handle
refresh, InitialisePose, the time advance through components, which draws are posed and where their slices lie."""
import numpy as np
import pytest

import anim_cases
import anim_ref
from trident_raster import abi, app

F = np.float32
IDENT = np.eye(4, dtype=np.float32).reshape(16)


def _rig(name):
    return next(r for r in anim_ref.kernel_rigs() if r.name == name)


@pytest.fixture()
def scene():
    a = app.TridentApp()
    a.set_camera("editor", (0.0, 1.0, 7.0))
    a.set_viewport(1, 64, 48)
    yield a
    a.close()


def test_update_resolves_handles_advances_time_and_writes_the_pose(scene):
    rig = _rig("chain3")
    h, clips = anim_cases.cpu_asset(rig)
    e = scene.add_mesh_entity("cube")
    scene.set_entity_animation(e, "test:chain3", "test:chain3", "slerp", time=0.25, speed=2.0)
    assert scene.entity_animation_state(e) == (0.25, True, None, None, None)
    scene.update_animation(0.125)
    assert scene.entity_animation_state(e) == (0.5, True, h, h, clips[1])
    assert np.array_equal(scene.entity_pose(e), app.anim_evaluate(h, clips[1], 0.5))
    scene.set_entity_animation(e, "test:chain3", "test:chain3", "slerp", time=0.9, looping=False)
    scene.update_animation(0.5)  # clamps at the duration and stops
    assert scene.entity_animation_state(e)[:2] == (1.0, False)
    scene.update_animation(0.5)  # paused: the time stays, the pose is refreshed
    assert scene.entity_animation_state(e)[:2] == (1.0, False)
    assert np.array_equal(scene.entity_pose(e), app.anim_evaluate(h, clips[1], 1.0))


def test_handles_follow_the_id_strings(scene):
    a3, c3 = anim_cases.cpu_asset(_rig("chain3"))
    fo, cf = anim_cases.cpu_asset(_rig("forest"))
    e = scene.add_mesh_entity("cube")
    scene.set_entity_animation(e, "test:chain3", "test:chain3", "hold")
    scene.update_animation(0.0)
    assert scene.entity_animation_state(e)[2:] == (a3, a3, c3[0])
    scene.set_entity_animation(e, "test:forest", "test:forest", "slerp")  # every id changed
    scene.update_animation(0.0)
    assert scene.entity_animation_state(e)[2:] == (fo, fo, cf[1])
    assert scene.entity_pose(e).shape == (6, 16)
    scene.set_entity_animation(e, "test:forest", "test:forest", "no such clip")
    scene.update_animation(0.0)
    assert scene.entity_animation_state(e)[2:] == (fo, fo, None)
    assert np.array_equal(scene.entity_pose(e), app.anim_evaluate(fo, None, 0.0))  # the bind pose
    scene.set_entity_animation(e, "test:not registered", None, None)
    scene.update_animation(0.0)
    assert scene.entity_animation_state(e)[2:] == (None, None, None)
    assert np.array_equal(scene.entity_pose(e), np.tile(IDENT, (6, 1)))  # the fallback keeps the last pose's size


def test_initialise_pose_and_entities_without_a_mesh(scene):
    rig = _rig("chain3")
    h, clips = anim_cases.cpu_asset(rig)
    e = scene.add_mesh_entity("cube")
    scene.set_entity_animation(e, "test:chain3", "test:chain3", "hold", time=0.7)
    scene.initialise_pose(e)  # time 0 of the clip, whatever the component's time
    assert np.array_equal(scene.entity_pose(e), app.anim_evaluate(h, clips[0], 0.0))
    assert scene.entity_animation_state(e)[0] == pytest.approx(0.7)
    light = scene.add_light("point")  # no MeshComponent: the system skips it
    scene.set_entity_animation(light, "test:chain3", "test:chain3", "hold", time=0.1)
    scene.update_animation(0.25)
    assert scene.entity_animation_state(light) == (pytest.approx(0.1), True, None, None, None)
    assert scene.entity_pose(light).shape == (0, 16)


def test_device_mode_lays_posed_draws_behind_the_uploaded_prefix(scene):
    """Host only (frame_inputs): with device poses on, draws with a valid skeleton handle take slices behind the draws
    that carry host matrices; a missing clip does not disqualify; an asset the device path refuses stays on the CPU."""
    h3, _ = anim_cases.cpu_asset(_rig("chain3"))
    h256, _ = anim_cases.cpu_asset(_rig("chain256"))
    bad = anim_ref.Rig("sys_decreasing", [-1, 0], np.tile(IDENT, (2, 1)), np.tile(IDENT, (2, 1)))
    bad.clips = [anim_ref.Clip("back", 1.0, [{"bone": 1, "T": (np.array([0.5, 0.25], F), np.zeros((2, 3), F)),
                                              "R": None, "S": None}])]
    anim_cases.cpu_asset(bad)
    e_posed = scene.add_mesh_entity("cube")
    e_host = scene.add_mesh_entity("cube", position=(2, 0, 0))
    e_big = scene.add_mesh_entity("cube", position=(-2, 0, 0))
    e_bad = scene.add_mesh_entity("cube", position=(0, 2, 0))
    e_plain = scene.add_mesh_entity("cube", position=(0, -2, 0))
    scene.set_entity_animation(e_posed, "test:chain3", "test:chain3", "absent clip")
    scene.set_entity_animation(e_big, "test:chain256", "test:chain256", "slerp", time=0.3)
    scene.set_entity_animation(e_bad, "test:sys_decreasing", "test:sys_decreasing", "back")

    def slices():
        # matrices written by other code, after the system ran (which gives a component without ids the fallback pose)
        scene.set_entity_bones(e_host, np.tile(IDENT, (5, 1)))
        _, draws = scene.frame_inputs(1)
        return [(d.pc.bone_offset, d.pc.bone_count) for d in draws]

    scene.frame_inputs(1)  # (the first frame creates the primitive meshes)
    scene.update_animation(0.0)  # CPU mode: every animated draw carries matrices, in draw order
    assert slices() == [(0, 3), (3, 5), (8, 128), (136, 2), (0, 0)]
    before = scene.bone_palette_uploads()
    scene.set_device_pose(True)
    scene.update_animation(0.125)  # time only
    assert scene.entity_animation_state(e_big)[0] == pytest.approx(0.425)
    # prefix: the host matrices (5) and the refused asset's CPU pose (2); then the posed draws, 3 and min(256, 128)
    assert slices() == [(7, 3), (0, 5), (10, 128), (5, 2), (0, 0)]
    assert scene.bone_palette_uploads() == before  # nothing was rendered
    assert np.array_equal(scene.entity_pose(e_big), app.anim_evaluate(h256, anim_cases.cpu_asset(_rig("chain256"))[1][1],
                                                                     scene.entity_animation_state(e_big)[0]))
    scene.set_device_pose(False)
    scene.update_animation(0.0)
    assert slices() == [(0, 3), (3, 5), (8, 128), (136, 2), (0, 0)]


def test_an_asset_registered_again_is_looked_at_again(scene):
    """Device poses follow the asset service's registrations: a skeleton replaced under its id changes the slice, an
    asset that stops being acceptable goes back to the CPU."""
    lb = np.tile(IDENT, (4, 1))
    app.anim_register("test:sys_again", [-1, 0, 1, 2], lb, lb)
    e = scene.add_mesh_entity("cube")
    scene.set_entity_animation(e, "test:sys_again", "test:sys_again", None)
    scene.set_device_pose(True)
    scene.frame_inputs(1)
    scene.update_animation(0.0)
    _, draws = scene.frame_inputs(1)
    assert (draws[0].pc.bone_offset, draws[0].pc.bone_count) == (0, 4)
    assert scene.entity_pose(e).shape == (4, 16)
    app.anim_register("test:sys_again", [-1, 0], lb[:2], lb[:2])  # replaced: two bones now
    scene.update_animation(0.0)
    _, draws = scene.frame_inputs(1)
    assert (draws[0].pc.bone_offset, draws[0].pc.bone_count) == (0, 2)
    app.anim_register("test:sys_again", [1, 0], lb[:2], lb[:2], root_index=0)  # a cycle: the device path refuses it
    scene.update_animation(0.0)  # ... so the CPU player evaluates it (its fallback pose) and the palette is uploaded
    _, draws = scene.frame_inputs(1)
    assert draws[0].pc.bone_count == scene.entity_pose(e).shape[0] > 0
