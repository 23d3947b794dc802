"""Animation state machines through the engine API on the GPU: a skinned mesh driven by a two-state machine with an
additive masked upper-body layer, next to a plain-clip entity and an entity with host-written matrices, renders the
same with Renderer::SetDevicePoseEnabled on (tri_pose_graph) as with the CPU system and the uploaded palette; with
frames in flight; and as row bands of a group."""
import numpy as np
import pytest

import anim_cases
import anim_graph_ref as G
import anim_ref
from trident_raster import app, scenes

pytestmark = pytest.mark.gpu

W, H = 96, 96
IDENT = np.eye(4, dtype=np.float32).reshape(16)
F = np.float32
DT = 0.0625  # the 0.2 s fade spans four updates


def _skinned_cube():
    """The primitive cube with every vertex on one of three bones by height."""
    v, i = scenes.cube_mesh()[:2]
    v = v.copy()
    y = v["position"][:, 1]
    v["bone_indices"][:, 0] = np.where(y > 0, 2, 1)
    v["bone_weights"][:] = 0.0
    v["bone_weights"][:, 0] = 1.0
    return v, i


def _track(values):
    v = np.array(values, F)
    return np.linspace(0.0, 1.0, len(v)).astype(F), v


def _quat(axis, deg):
    h = np.radians(deg) / 2
    return [np.cos(h)] + [np.sin(h) * a for a in axis]


def _asset():
    """Three bones in a column with identity rest rotations (an additive layer then multiplies identities: every slerp
    of the translation / scale clips takes its linear branch, and the device palette equals the CPU one bit for bit).
    Clips 0-2 "idle", "walk", "lean" animate translation and scale only; clips 3-5 are the same with rotations."""
    lb = np.stack([anim_ref.compose([0.0, 0.2 * (b > 0), 0.0], [1, 0, 0, 0], [1, 1, 1]) for b in range(3)]).astype(F)
    rig = anim_ref.Rig("sm_shim", [-1, 0, 1], lb, np.tile(IDENT, (3, 1)))
    ts = {"idle": [{"bone": 1, "T": _track([[0, 0.2, 0], [0.1, 0.25, 0], [0, 0.2, 0]]), "R": None, "S": None},
                   {"bone": 2, "T": None, "R": None, "S": _track([[1, 1, 1], [1.1, 0.9, 1.1], [1, 1, 1]])}],
          "walk": [{"bone": 1, "T": _track([[0.3, 0.2, 0], [-0.3, 0.3, 0.1], [0.3, 0.2, 0]]), "R": None, "S": None},
                   {"bone": 2, "T": _track([[0, 0.2, 0.2], [0, 0.3, -0.2]]), "R": None, "S": None}],
          "lean": [{"bone": 2, "T": _track([[0.2, 0, 0], [0.4, 0.1, 0]]), "R": None, "S": None}]}
    rot = {"idle": _track([_quat((0, 0, 1), 0), _quat((0, 0, 1), 25)]), "walk": _track([_quat((1, 0, 0), -30), _quat((1, 0, 0), 40)]),
           "lean": _track([_quat((0, 1, 0), 10), _quat((0, 1, 0), 70)])}
    rig.clips = [anim_ref.Clip(n, 1.0, ts[n]) for n in ("idle", "walk", "lean")]
    rig.clips += [anim_ref.Clip(n + "_r", 1.0, ts[n] + [{"bone": 1 if n != "lean" else 2, "T": None, "R": rot[n], "S": None}])
                  for n in ("idle", "walk", "lean")]
    return anim_cases.cpu_asset(rig)


def _machine(rotating):
    k = 3 if rotating else 0
    sm = app.StateMachine(None)
    base = sm.add_layer("base")
    sm.add_state(base, "idle", app.node_clip(k + 0))
    sm.add_state(base, "walk", app.node_clip(k + 1, speed=1.5))
    sm.set_layer_entry(base, "idle")
    sm.add_parameter("go", app.SM_TRIGGER)
    sm.add_transition(base, "idle", "walk", fade=0.2, conditions=[("go", "triggered", 0)])
    upper = sm.add_layer("upper", 0.5, additive=True)
    sm.add_state(upper, "lean", app.node_clip(k + 2))
    sm.set_layer_entry(upper, "lean")
    sm.set_layer_mask(upper, [0.0, 0.0, 1.0])
    return sm


def _scene(device_pose, rotating, frames_in_flight=1, devices=None):
    _asset()
    a = app.TridentApp()
    if devices:
        a.set_device_count(len(devices), devices)
    a.set_frames_in_flight(frames_in_flight)
    a.set_camera("editor", (0.0, 0.5, 6.0))
    a.set_viewport(1, W, H)
    a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=4.0)
    mesh = a.append_mesh(*_skinned_cube())
    ents = [a.add_mesh_entity("none", mesh, position=(x, 0.0, 0.0), rotation=(20.0, 30.0, 0.0)) for x in (-2.0, 0.0, 2.0)]
    # a state machine, a plain clip, and matrices written by other code (the uploaded prefix)
    a.set_entity_animation(ents[0], "test:sm_shim", "test:sm_shim", None)
    a.set_entity_animation(ents[1], "test:sm_shim", "test:sm_shim", "walk_r" if rotating else "walk", time=0.1)
    sm = _machine(rotating)
    a.set_entity_state_machine(ents[0], sm)
    a.set_device_pose(device_pose)
    return a, ents, sm


def _step(a, ents, sm, k):
    host = np.tile(IDENT, (3, 1))
    host[2, 12] = 0.5
    if k == 1:
        sm.fire("go")
    a.update_animation(DT)
    a.set_entity_bones(ents[2], host)
    a.draw_frame()


def _frames(a, ents, sm, n):
    out = []
    for k in range(n):
        _step(a, ents, sm, k)
        a.finish_frame()
        out.append(a.read_pixels(1, W, H))
    return out


def _close(*scenes):
    for a, _, sm in scenes:
        a.close()
        sm.close()


def test_translation_scale_machine_renders_the_cpu_frames_without_palette_uploads():
    cpu, dev = _scene(False, False), _scene(True, False)
    fc, fd = _frames(*cpu, 7), _frames(*dev, 7)
    for k, ((pc, zc), (pd, zd)) in enumerate(zip(fc, fd)):
        assert np.array_equal(zc, zd) and np.array_equal(pc, pd), f"frame {k}"
    assert not np.array_equal(fc[0][0], fc[3][0]) and not np.array_equal(fc[3][0], fc[6][0])
    assert (fc[0][1] != 1.0).sum() > 3 * 10 * 10  # three cubes of about 14 pixels are on screen
    # the fade ran: walk is the current state by the last frame, on both paths
    assert cpu[2].layer_state(0)[:2] == dev[2].layer_state(0)[:2] == ("walk", "")
    assert cpu[0].bone_palette_uploads() == 7  # a new palette every frame
    assert dev[0].bone_palette_uploads() == 1  # the static prefix once
    # host code that reads the pose gets the CPU evaluation of the machine's current program
    ops, masks = dev[2].program()
    assert ops[-1][0] == G.ADD and [m.tolist() for m in masks] == [[0.0, 0.0, 1.0]]
    handle, _ = _asset()
    assert np.array_equal(dev[0].entity_pose(dev[1][0]), app.anim_eval_program(handle, ops, masks))
    assert np.array_equal(dev[0].entity_pose(dev[1][0]), cpu[0].entity_pose(cpu[1][0]))
    _close(cpu, dev)


def test_rotating_machine_is_within_one_lsb():
    cpu, dev = _scene(False, True), _scene(True, True)
    fc, fd = _frames(*cpu, 6), _frames(*dev, 6)
    for k, ((pc, zc), (pd, zd)) in enumerate(zip(fc, fd)):
        diff = int(np.abs(pc.astype(np.int16) - pd.astype(np.int16)).max())
        print(f"frame {k}: max colour difference {diff} LSB, depth words differing {int((zc != zd).sum())}")
        assert diff <= 1, f"frame {k}"
    assert not np.array_equal(fc[0][0], fc[5][0])
    assert dev[0].bone_palette_uploads() == 1
    _close(cpu, dev)


def test_frames_in_flight_and_row_bands():
    ref = _scene(False, False)
    want = _frames(*ref, 6)[-1]
    ring = _scene(True, False, frames_in_flight=3)
    for k in range(6):  # no wait between frames: each ring target is posed for its own frame
        _step(*ring, k)
    ring[0].finish_frame()
    got = ring[0].read_pixels(1, W, H)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    bands = _scene(True, False, devices=[0, 0])  # a group of two bands: tri_group_pose_graph
    got = _frames(*bands, 6)[-1]
    assert np.array_equal(got[1], want[1])
    assert int(np.abs(got[0].astype(np.int16) - want[0].astype(np.int16)).max()) <= 1
    assert bands[0].bone_palette_uploads() == 1
    _close(ref, ring, bands)


def test_a_program_the_device_refuses_is_evaluated_on_the_cpu():
    """A state whose blend tree nests nine clips deep exceeds TRI_POSE_STACK: that component joins the uploaded prefix,
    the plain clip next to it stays on the device, and the frame is the CPU path's."""
    def deep(a, ents):
        sm = app.StateMachine(None)
        layer = sm.add_layer("base")
        node = app.node_clip(0)
        for i in range(9):  # right-nested: the second child is the deeper tree
            node = app.node_blend(app.node_clip(i % 3), node, 0.5)
        sm.add_state(layer, "deep", node)
        sm.set_layer_entry(layer, "deep")
        a.set_entity_state_machine(ents[0], sm)
        return sm

    frames = {}
    for mode in (False, True):
        a, ents, first = _scene(mode, False)
        sm = deep(a, ents)
        frames[mode] = _frames(a, ents, sm, 2)
        assert a.bone_palette_uploads() == 2  # on either path a palette with the machine's matrices, every frame
        _close((a, ents, sm))
        first.close()
    for (pc, zc), (pd, zd) in zip(frames[False], frames[True]):
        assert np.array_equal(zc, zd) and np.array_equal(pc, pd)
