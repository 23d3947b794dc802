"""The glTF skin / animation reader against the fixture's own expectations (tests/golden/anim/rig_expected.json, written
beside rig.gltf by tests/golden/make_anim_fixture.py): bones, parents, root, inverse binds, vertex influences, clips;
the asset service loading a model file once per id; damaged copies refused; skinless models as before."""
import base64
import json
import os

import numpy as np
import pytest

from trident_raster import app

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RIG = os.path.join(ROOT, "tests", "golden", "anim", "rig.gltf")
F = np.float32
IDENT = np.eye(4, dtype=np.float32).reshape(16)


def _f32(obj):
    """Every float of a JSON tree as the float32 it stands for (the shim prints 9 significant digits, which name one)."""
    if isinstance(obj, float):
        return float(F(obj))
    if isinstance(obj, list):
        return [_f32(v) for v in obj]
    if isinstance(obj, dict):
        return {k: _f32(v) for k, v in obj.items()}
    return obj


@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(ROOT, "tests", "golden", "anim", "rig_expected.json")) as f:
        return _f32(json.load(f))


@pytest.fixture(scope="module")
def rig():
    h = app.anim_load(RIG)
    assert h is not None
    return h, _f32(app.anim_describe(h))


def test_bones_parents_root_and_inverse_binds(rig, expected):
    _, got = rig
    assert got["root"] == expected["root"] == 0
    assert [b["source"] for b in got["bones"]] == ["Root", "mixamorig:Arm", "Hand", "Node4", "Tail", "Extra", "Prop"]
    for g, e in zip(got["bones"], expected["bones"]):
        assert (g["source"], g["name"], g["parent"], g["children"]) == (e["source"], e["name"], e["parent"], e["children"])
        assert g["inverse"] == e["inverse"], g["source"]  # float32 values straight from the accessor
        # the node's T * R * S, evaluated in float32 here and in float64 by the fixture script
        assert np.abs(np.array(g["local"]) - np.array(e["local"])).max() <= 4e-7, g["source"]
    by = {b["source"]: b for b in got["bones"]}
    assert by["mixamorig:Arm"]["parent"] == 0  # the Spacer node in between is no bone: its transform is dropped
    assert by["Extra"]["inverse"] == IDENT.tolist() and by["Prop"]["inverse"] == IDENT.tolist()
    assert by["Prop"]["parent"] == 2 and by["Node4"]["name"] == "Node4" and by["mixamorig:Arm"]["name"] == "Arm"


def test_clips(rig, expected):
    h, got = rig
    assert [c["name"] for c in got["clips"]] == ["Walk", "Clip1", "Bend"]
    assert got["clips"] == expected["clips"]  # durations, ticks, channel order, bones, source names, every key
    walk = got["clips"][0]
    assert [len(walk["channels"][0][k]) for k in "trs"] == [2, 3, 4]
    assert walk["channels"][2]["t"] == [[0.0, 0.0, 0.5, 0.0], [2.0, 0.0, 0.75, 0.0]]  # CUBICSPLINE: the value elements
    assert [c["bone"] for c in got["clips"][1]["channels"]] == [0, 0]  # one bone, two channels; no morph channel
    assert app.anim_clip_index(h, "Clip1") == 1
    assert app.anim_resolve_channels(h, 0).tolist() == [1, 2, 3, 6]
    # the later channel wins: the root sits at its second channel's key
    assert app.anim_evaluate(h, 1, 1.0)[0][13] == pytest.approx(0.5)


def test_vertex_influences(expected):
    a = app.TridentApp()
    ents = a.import_model(RIG)
    assert len(ents) == 2
    vb, _, ranges = a.geometry()
    a.close()
    assert len(vb) == 27
    want = {tuple(i["position"]): {int(b): w for b, w in i["bones"].items()} for i in expected["influences"]}
    assert len(want) == 27
    for v in vb:
        got = {int(b): float(w) for b, w in zip(v["bone_indices"], v["bone_weights"]) if w > 0}
        assert got == want[tuple(float(x) for x in v["position"])]
        assert abs(sum(got.values()) - 1.0) <= 2e-7


def test_bind_pose_of_the_loaded_rig_moves_nothing_the_skin_binds(rig):
    """pose = global * inverse bind at the bind pose: the identity up to the dropped Spacer transform (0.25 in x below
    it) for skin 0's joints."""
    h, got = rig
    pose = app.anim_evaluate(h, None, 0.0)
    for b, bone in enumerate(got["bones"][:5]):
        want = IDENT.copy()
        if bone["source"] in ("mixamorig:Arm", "Hand", "Node4"):
            want[12] = -0.25
        assert np.abs(pose[b] - want).max() <= 1e-6, bone["source"]


def test_a_file_is_loaded_once_per_id_and_missing_ones_warn_once(tmp_path, capfd):
    path = tmp_path / "copy.gltf"
    path.write_text(open(RIG).read())
    h = app.anim_load(str(path))
    assert h is not None and h != app.anim_load(RIG)
    path.unlink()  # the id is known: nothing is read again
    assert app.anim_load(str(path)) == h
    a = app.TridentApp()
    e = a.add_mesh_entity("cube")
    missing = str(tmp_path / "absent.gltf")
    a.set_entity_animation(e, missing, missing, "Walk")
    capfd.readouterr()
    for _ in range(3):
        a.update_animation(0.1)
    assert capfd.readouterr().err.count("could not be loaded") == 1
    a.set_entity_animation(e, RIG, RIG, "Bend", time=0.5)  # an id that is a model file: loaded through the service
    a.update_animation(0.0)
    t, playing, sk, an, clip = a.entity_animation_state(e)
    assert (sk, an, clip) == (app.anim_load(RIG), app.anim_load(RIG), 2)
    assert a.entity_pose(e).shape == (7, 16)
    a.close()


def _damaged(tmp_path, name, edit):
    g = json.load(open(RIG))
    blob = bytearray(base64.b64decode(g["buffers"][0]["uri"].split(",", 1)[1]))
    blob = edit(g, blob) or blob
    g["buffers"][0]["uri"] = "data:application/octet-stream;base64," + base64.b64encode(bytes(blob)).decode()
    g["buffers"][0]["byteLength"] = len(blob)
    path = tmp_path / name
    path.write_text(json.dumps(g))
    return str(path)


def _joint_beyond(g, blob):
    view = g["bufferViews"][g["accessors"][g["meshes"][0]["primitives"][0]["attributes"]["JOINTS_0"]]["bufferView"]]
    blob[view["byteOffset"]] = 200


def _counts_disagree(g, blob):
    g["accessors"][g["animations"][0]["samplers"][1]["output"]]["count"] = 2


def _truncated(g, blob):
    return blob[:len(blob) // 2]


def _short_inverse_binds(g, blob):
    g["accessors"][g["skins"][0]["inverseBindMatrices"]]["count"] = 3


@pytest.mark.parametrize("edit", [_joint_beyond, _counts_disagree, _truncated, _short_inverse_binds])
def test_damaged_files_are_refused_with_a_message(tmp_path, capfd, edit):
    path = _damaged(tmp_path, edit.__name__ + ".gltf", edit)
    capfd.readouterr()
    assert app.anim_load(path) is None
    assert "glTF" in capfd.readouterr().err
    a = app.TridentApp()
    with pytest.raises(app.TriError):  # no half-read model either: the import fails as for any unreadable file
        a.import_model(path)
    a.close()


def test_a_300_bone_skin_loads_and_stays_on_the_cpu(tmp_path):
    g = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}],
         "nodes": [{"name": f"J{i}", "translation": [0, 0.01, 0], **({"children": [i + 1]} if i < 299 else {})}
                   for i in range(300)],
         "skins": [{"joints": list(range(300))}]}
    path = tmp_path / "chain300.gltf"
    path.write_text(json.dumps(g))
    h = app.anim_load(str(path))
    d = app.anim_describe(h)
    assert len(d["bones"]) == 300 and d["bones"][299]["parent"] == 298 and d["root"] == 0
    pose = app.anim_evaluate(h, None, 0.0)
    assert pose.shape == (300, 16) and pose[299][13] == pytest.approx(3.0, abs=1e-4)


def test_skinless_models_yield_no_skeleton_and_unweighted_vertices(tmp_path):
    g = json.load(open(RIG))
    for key in ("skins", "animations"):
        del g[key]
    for n in g["nodes"]:
        n.pop("skin", None)
    plain = tmp_path / "plain.gltf"
    plain.write_text(json.dumps(g))
    assert app.anim_load(str(plain)) is None
    a, b = app.TridentApp(), app.TridentApp()
    assert len(a.import_model(str(plain))) == 2 and len(b.import_model(RIG)) == 2
    va, ia, _ = a.geometry()
    vb, ib, _ = b.geometry()
    a.close()
    b.close()
    assert not va["bone_weights"].any() and not va["bone_indices"].any()
    # the skin changes nothing else about the mesh: same vertices in the same order, same indices
    for field in ("position", "normal", "tangent", "bitangent", "color", "texcoord"):
        assert np.array_equal(va[field], vb[field]), field
    assert np.array_equal(ia, ib)
    obj = tmp_path / "tri.obj"
    obj.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert app.anim_load(str(obj)) is None
