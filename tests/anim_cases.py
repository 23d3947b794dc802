"""Glue the animation tests share: a rig of tests/anim_ref.py registered with the shim's CPU asset service, and added
to a device tri_animset, from the same float32 arrays."""
import numpy as np

from trident_raster import abi, app

_CPU = {}


def channel_rows(clip, bones=None):
    rows, vt, vv, qt, qv = clip.flat()
    ch = np.zeros(len(rows), abi.POSE_CHANNEL_DTYPE)
    for i, r in enumerate(rows):
        ch[i] = (r[0] if bones is None else bones[i], r[1], r[2], r[3], r[4], r[5], r[6], 0)
    return ch, vt, vv, qt, qv


def defaults(rig):
    """Per bone (translation, rotation, scale): the shim's float32 DecomposeBindTransform."""
    return [app.anim_decompose(rig.local_binds[b]) for b in range(rig.bones)]


def cpu_asset(rig):
    """(handle, [clip index per rig.clips]) in the shim's asset service, registered once per rig name."""
    if rig.name not in _CPU:
        h = app.anim_register("test:" + rig.name, rig.parents, rig.local_binds, rig.inverse_binds, rig.source_names,
                              rig.root_index)
        clips = []
        for clip in rig.clips:
            ch, vt, vv, qt, qv = channel_rows(clip)
            clips.append(app.anim_add_clip(h, clip.name, clip.duration, ch, vt, vv, qt, qv))
        _CPU[rig.name] = (h, clips)
    return _CPU[rig.name]


def pose_bones(rig):
    b = np.zeros(rig.bones, abi.POSE_BONE_DTYPE)
    for i, (t, r, s) in enumerate(defaults(rig)):
        b[i]["parent"] = rig.parents[i]
        b[i]["translation"][:3] = t
        b[i]["rotation"] = r
        b[i]["scale"][:3] = s
        b[i]["inverse_bind"] = rig.inverse_binds[i]
    return b


def device_asset(animset, rig):
    """(skeleton, [clip per rig.clips]) in a raster.TriAnimSet."""
    sk = animset.add_skeleton(pose_bones(rig), rig.root_index)
    clips = []
    for clip in rig.clips:
        ch, vt, vv, qt, qv = channel_rows(clip)
        clips.append(animset.add_clip(sk, ch, vt, vv, qt, qv, clip.duration))
    return sk, clips
