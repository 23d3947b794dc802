#!/usr/bin/env python3
"""Writes tests/golden/anim/rig.gltf (one embedded buffer) and rig_expected.json: what the glTF skin / animation
reader must make of it, by the rules in host/include/trident/ModelLoader.h.

The rig: a 24-vertex two-segment bar (6 rings of 4 corners along y) skinned to the 5 joints of skin 0, with a node that
is no joint between two of them; a triangle under a second skin that shares 3 of those joints and adds one; one
animated node that is no joint. Three clips: "Walk" drives all three tracks of the `mixamorig:`-prefixed joint LINEAR
with 2 / 3 / 4 keys, one STEP rotation, one CUBICSPLINE translation and the animated non-joint; an unnamed one gives
one bone two channels and carries a morph-target channel, which is skipped; "Bend" is what the GPU tests play.

    python tests/golden/make_anim_fixture.py
"""
import base64
import json
import os
import struct

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "anim")
F = np.float32


def trs(t=(0, 0, 0), q=(0, 0, 0, 1), s=(1, 1, 1)):
    """glTF's T * R * S as a column-major float64 [4, 4] indexed [column][row]; q is x, y, z, w."""
    x, y, z, w = q
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)],
                  [2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)],
                  [2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)]])
    m = np.zeros((4, 4))
    for j in range(3):
        m[j][:3] = r[j] * s[j]
    m[3] = [t[0], t[1], t[2], 1.0]
    return m


# node index: (name, parent node, translation, rotation x y z w, scale)
H = float(np.sqrt(0.5))
NODES = [
    ("Root", None, (0.0, -1.0, 0.0), (0, 0, 0, 1), (1, 1, 1)),           # 0 joint
    ("Spacer", 0, (0.25, 0.0, 0.0), (0, 0, 0, 1), (1, 1, 1)),            # 1 no joint: its transform is dropped
    ("mixamorig:Arm", 1, (0.0, 0.5, 0.0), (0, 0, H, H), (1, 1, 1)),      # 2 joint
    ("Hand", 2, (0.0, 0.5, 0.0), (0, 0, 0, 1), (1, 2, 1)),               # 3 joint
    (None, 3, (0.0, 0.5, 0.0), (0, 0, 0, 1), (1, 1, 1)),                 # 4 joint without a name: "Node4"
    ("Tail", 0, (0.0, -0.5, 0.0), (0, 0, 0, 1), (1, 1, 1)),              # 5 joint
    ("Prop", 3, (0.5, 0.0, 0.0), (0, 0, 0, 1), (1, 1, 1)),               # 6 animated, no joint
    ("Bar", None, (0, 0, 0), (0, 0, 0, 1), (1, 1, 1)),                   # 7 mesh 0, skin 0
    ("Flag", None, (0, 0, 0), (0, 0, 0, 1), (1, 1, 1)),                  # 8 mesh 1, skin 1
    ("Extra", 0, (0.0, 0.0, 0.5), (0, 0, 0, 1), (1, 1, 1)),              # 9 joint of skin 1 only
]
SKINS = [[0, 2, 3, 4, 5], [3, 4, 0, 9]]
# bones: skin 0's joints, skin 1's unseen joint, then the animated non-joint
BONE_NODES = [0, 2, 3, 4, 5, 9, 6]


class Buffer:
    def __init__(self):
        self.data, self.views, self.accessors = bytearray(), [], []

    def add(self, array, ctype, kind, normalized=False, minmax=False):
        a = np.ascontiguousarray(array)
        while len(self.data) % 4:
            self.data.append(0)
        self.views.append({"buffer": 0, "byteOffset": len(self.data), "byteLength": a.nbytes})
        self.data += a.tobytes()
        acc = {"bufferView": len(self.views) - 1, "componentType": ctype, "count": int(a.shape[0]), "type": kind}
        if normalized:
            acc["normalized"] = True
        if minmax:
            acc["min"], acc["max"] = a.min(axis=0).tolist(), a.max(axis=0).tolist()
        self.accessors.append(acc)
        return len(self.accessors) - 1


def node_global(n):
    name, parent, t, q, s = NODES[n]
    m = trs(t, q, s)
    return m if parent is None else m @ node_global(parent)  # [column][row] arrays: parent * local


def main():
    os.makedirs(OUT, exist_ok=True)
    buf = Buffer()
    # the bar: 6 rings of 4 corners at y = -1.5 .. 1.0, weights sliding from one joint slot to the next
    rings = np.linspace(-1.5, 1.0, 6)
    corners = [(-0.1, -0.1), (0.1, -0.1), (0.1, 0.1), (-0.1, 0.1)]
    pos = np.array([(x, y, z) for y in rings for x, z in corners], F)
    nrm = np.array([(x * 10 * H, 0.0, z * 10 * H) for _ in rings for x, z in corners], F)
    slots = [(4, 0, 1.0), (0, 1, 0.75), (0, 1, 0.25), (1, 2, 0.5), (2, 3, 0.5), (3, 3, 1.0)]  # (slot a, slot b, weight a)
    joints = np.zeros((24, 4), np.uint8)
    weights = np.zeros((24, 4), F)
    for r, (a, b, wa) in enumerate(slots):
        for c in range(4):
            v = 4 * r + c
            if a == b or wa == 1.0:
                joints[v], weights[v] = (a, 0, 0, 0), (2.0, 0, 0, 0)  # one influence, not normalised in the file
            else:
                joints[v], weights[v] = (a, b, 0, 0), (wa, 1.0 - wa, 0, 0)
    idx = []
    for r in range(5):
        for c in range(4):
            a, b = 4 * r + c, 4 * r + (c + 1) % 4
            idx += [a, b, a + 4, b, b + 4, a + 4]
    mesh0 = {"attributes": {"POSITION": buf.add(pos, 5126, "VEC3", minmax=True), "NORMAL": buf.add(nrm, 5126, "VEC3"),
                            "JOINTS_0": buf.add(joints, 5121, "VEC4"), "WEIGHTS_0": buf.add(weights, 5126, "VEC4")},
             "indices": buf.add(np.array(idx, np.uint16), 5123, "SCALAR")}
    # the flag: one triangle, u16 joints into skin 1, normalised u8 weights, five influences' worth squeezed into four
    fpos = np.array([(0.5, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 0.5, 0.0)], F)
    fnrm = np.array([(0, 0, 1)] * 3, F)
    fj = np.array([(0, 1, 2, 3), (3, 0, 0, 0), (2, 1, 0, 0)], np.uint16)
    fw = np.array([(51, 102, 51, 51), (255, 0, 0, 0), (128, 64, 0, 0)], np.uint8)
    mesh1 = {"attributes": {"POSITION": buf.add(fpos, 5126, "VEC3", minmax=True), "NORMAL": buf.add(fnrm, 5126, "VEC3"),
                            "JOINTS_0": buf.add(fj, 5123, "VEC4"),
                            "WEIGHTS_0": buf.add(fw, 5121, "VEC4", normalized=True)}}
    # inverse binds: the inverse of each joint node's global transform (non-joint nodes in between included, as an
    # exporter writes them), float32
    ibm = [np.stack([np.linalg.inv(node_global(n)).reshape(16) for n in js]).astype(F) for js in SKINS]
    skins = [{"joints": SKINS[0], "inverseBindMatrices": buf.add(ibm[0], 5126, "MAT4")},
             {"joints": SKINS[1]}]  # the second skin has no accessor: its new joint gets the identity

    def sampler(times, values, kind, interp=None):
        s = {"input": buf.add(np.array(times, F), 5126, "SCALAR", minmax=True), "output": buf.add(np.array(values, F), 5126, kind)}
        if interp:
            s["interpolation"] = interp
        return s

    q90 = (0, 0, H, H)
    walk_s = [
        sampler([0.0, 1.0], [(0, 0.5, 0), (0.2, 0.5, 0)], "VEC3"),                                   # 0 arm T, 2 keys
        sampler([0.0, 0.5, 1.0], [q90, (0, 0, 0, 1), (0, 0, -H, H)], "VEC4", "LINEAR"),              # 1 arm R, 3 keys
        sampler([0.0, 0.25, 0.5, 1.0], [(1, 1, 1), (1, 1.5, 1), (1, 1, 1), (2, 1, 1)], "VEC3"),      # 2 arm S, 4 keys
        sampler([0.0, 0.5], [(0, 0, 0, 1), (H, 0, 0, H)], "VEC4", "STEP"),                           # 3 hand R
        sampler([0.0, 2.0], [(9, 9, 9), (0, 0.5, 0), (9, 9, 9), (8, 8, 8), (0, 0.75, 0), (8, 8, 8)], "VEC3", "CUBICSPLINE"),  # 4
        sampler([0.5, 1.5], [(0.5, 0, 0), (0.5, 0.5, 0)], "VEC3"),                                   # 5 prop T
    ]
    walk_c = [(0, 2, "translation"), (1, 2, "rotation"), (2, 2, "scale"), (3, 3, "rotation"), (4, 4, "translation"),
              (5, 6, "translation")]
    two_s = [sampler([0.0], [(0, -1, 0)], "VEC3"), sampler([0.0, 1.0], [(0, -1, 0), (0, -0.5, 0)], "VEC3"),
             sampler([0.0], [(1.0,)], "SCALAR")]
    two_c = [(0, 0, "translation"), (1, 0, "translation"), (2, 7, "weights")]
    bend_s = [sampler([0.0, 1.0, 2.0], [(0, 0, 0, 1), (0, 0, 0.5, 0.8660254), (0, 0, 0, 1)], "VEC4"),
              sampler([0.0, 2.0], [(0, 0.5, 0), (0.1, 0.5, 0)], "VEC3")]
    bend_c = [(0, 3, "rotation"), (1, 2, "translation")]

    def anim(name, samplers, channels):
        a = {"samplers": samplers, "channels": [{"sampler": s, "target": {"node": n, "path": p}} for s, n, p in channels]}
        if name:
            a["name"] = name
        return a

    animations = [anim("Walk", walk_s, walk_c), anim(None, two_s, two_c), anim("Bend", bend_s, bend_c)]
    nodes = []
    for i, (name, parent, t, q, s) in enumerate(NODES):
        n = {"translation": list(t), "rotation": list(q), "scale": list(s)}
        if name:
            n["name"] = name
        kids = [k for k, other in enumerate(NODES) if other[1] == i]
        if kids:
            n["children"] = kids
        nodes.append(n)
    nodes[7].update(mesh=0, skin=0)
    nodes[8].update(mesh=1, skin=1)
    gltf = {"asset": {"version": "2.0", "generator": "make_anim_fixture.py"}, "scene": 0,
            "scenes": [{"nodes": [0, 7, 8]}], "nodes": nodes,
            "meshes": [{"primitives": [mesh0]}, {"primitives": [mesh1]}], "skins": skins, "animations": animations,
            "accessors": buf.accessors, "bufferViews": buf.views,
            "buffers": [{"byteLength": len(buf.data),
                         "uri": "data:application/octet-stream;base64," + base64.b64encode(bytes(buf.data)).decode()}]}
    with open(os.path.join(OUT, "rig.gltf"), "w") as f:
        json.dump(gltf, f, separators=(",", ":"))
        f.write("\n")

    # ---- what the reader must make of it ----
    def f32(a):
        return [float(F(v)) for v in np.asarray(a, np.float64).reshape(-1)]

    bone_of = {n: b for b, n in enumerate(BONE_NODES)}
    bones = []
    for b, n in enumerate(BONE_NODES):
        name, parent, t, q, s = NODES[n]
        source = name or f"Node{n}"
        up = parent
        while up is not None and up not in bone_of:
            up = NODES[up][1]
        inverse = np.eye(4).reshape(16)
        if n in SKINS[0]:
            inverse = ibm[0][SKINS[0].index(n)]
        bones.append({"source": source, "name": source.strip().removeprefix("mixamorig:"),
                      "parent": -1 if up is None else bone_of[up],
                      "local": f32(trs(F(t).astype(np.float64), F(q).astype(np.float64), F(s).astype(np.float64))),
                      "inverse": f32(inverse)})
    for b, bone in enumerate(bones):
        bone["children"] = [c for c, other in enumerate(bones) if other["parent"] == b]

    def keys(times, values, rotation=False, cubic=False):
        vals = values[1::3] if cubic else values
        return [[float(F(t))] + f32((v[3], v[0], v[1], v[2]) if rotation else v) for t, v in zip(times, vals)]

    def channel(node, t=None, r=None, s=None):
        return {"bone": bone_of[node], "source": bones[bone_of[node]]["source"], "t": t or [], "r": r or [], "s": s or []}

    clips = [
        {"name": "Walk", "duration": 2.0, "ticks": 1000.0, "channels": [
            channel(2, keys([0.0, 1.0], [(0, 0.5, 0), (0.2, 0.5, 0)]),
                    keys([0.0, 0.5, 1.0], [q90, (0, 0, 0, 1), (0, 0, -H, H)], rotation=True),
                    keys([0.0, 0.25, 0.5, 1.0], [(1, 1, 1), (1, 1.5, 1), (1, 1, 1), (2, 1, 1)])),
            channel(3, r=keys([0.0, 0.5], [(0, 0, 0, 1), (H, 0, 0, H)], rotation=True)),
            channel(4, t=keys([0.0, 2.0], [(9, 9, 9), (0, 0.5, 0), (9, 9, 9), (8, 8, 8), (0, 0.75, 0), (8, 8, 8)], cubic=True)),
            channel(6, t=keys([0.5, 1.5], [(0.5, 0, 0), (0.5, 0.5, 0)]))]},
        {"name": "Clip1", "duration": 1.0, "ticks": 1000.0, "channels": [
            channel(0, t=keys([0.0], [(0, -1, 0)])), channel(0, t=keys([0.0, 1.0], [(0, -1, 0), (0, -0.5, 0)]))]},
        {"name": "Bend", "duration": 2.0, "ticks": 1000.0, "channels": [
            channel(3, r=keys([0.0, 1.0, 2.0], [(0, 0, 0, 1), (0, 0, 0.5, 0.8660254), (0, 0, 0, 1)], rotation=True)),
            channel(2, t=keys([0.0, 2.0], [(0, 0.5, 0), (0.1, 0.5, 0)]))]},
    ]
    # vertex influences by position, as {bone: weight} after AssignBoneWeight / NormaliseBoneWeights
    influences = []
    for v in range(24):
        raw = [(bone_of[SKINS[0][int(j)]], float(w)) for j, w in zip(joints[v], weights[v]) if w > 0]
        total = F(0.0)
        for _, w in raw:
            total = F(total + F(w))
        influences.append({"position": f32(pos[v]), "bones": {str(b): float(F(F(w) * (F(1.0) / total))) for b, w in raw}})
    for v in range(3):
        w = (fw[v].astype(F) / F(255.0))
        raw = [(bone_of[SKINS[1][int(j)]], w[k]) for k, j in enumerate(fj[v]) if w[k] > 0]
        total = F(0.0)
        for _, x in raw:
            total = F(total + x)
        influences.append({"position": f32(fpos[v]), "bones": {str(b): float(F(x * (F(1.0) / total))) for b, x in raw}})
    expected = {"root": 0, "bones": bones, "clips": clips, "influences": influences}
    with open(os.path.join(OUT, "rig_expected.json"), "w") as f:
        json.dump(expected, f, indent=1)
        f.write("\n")
    print("wrote", os.path.join(OUT, "rig.gltf"), len(buf.data), "buffer bytes")


if __name__ == "__main__":
    main()
