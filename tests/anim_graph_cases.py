"""Glue the pose-graph tests share: the graph rigs of tests/anim_graph_ref.py registered with the shim and added to a
device tri_animset (through tests/anim_cases.py), and programs translated into either implementation's ids."""
import numpy as np

import anim_cases
import anim_graph_ref as G
from trident_raster import abi, app

assert (G.REST, G.CLIP, G.BLEND, G.ADD) == (abi.TRI_POSE_OP_REST, abi.TRI_POSE_OP_CLIP, abi.TRI_POSE_OP_BLEND,
                                            abi.TRI_POSE_OP_ADD)
assert (G.NO_MASK, G.STACK, G.MAX_OPS) == (abi.TRI_POSE_NO_MASK, abi.TRI_POSE_STACK, abi.TRI_POSE_MAX_OPS)


def cpu_ops(ops, cpu_clips):
    """ops with clip positions replaced by the shim asset's clip indices (masks stay positions in the mask list)."""
    return [(op, cpu_clips[a] if op == G.CLIP else a, f) for op, a, f in ops]


def cpu_matrices(rig, ops, masks):
    """The shim's float32 interpreter on a graph rig: float32 [bones, 16]."""
    h, cpu_clips = anim_cases.cpu_asset(rig)
    return app.anim_eval_program(h, cpu_ops(ops, cpu_clips), masks)


def device_asset(animset, rig):
    """(skeleton, [clip per rig.clips], [mask per masks_for(rig)]) in a raster.TriAnimSet."""
    sk, clips = anim_cases.device_asset(animset, rig)
    return sk, clips, [animset.add_mask(sk, m) for m in G.masks_for(rig)]


def device_ops(ops, clips, masks):
    out = np.zeros(len(ops), abi.POSE_OP_DTYPE)
    for i, (op, a, f) in enumerate(ops):
        if op == G.CLIP:
            a = clips[a]
        elif op in (G.BLEND, G.ADD) and a != G.NO_MASK:
            a = masks[a]
        out[i] = (op, a, f, 0)
    return out
