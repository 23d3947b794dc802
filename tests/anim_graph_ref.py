"""The pose-space rules of include/tri_raster.h ("Pose space", "A pose program") restated in float64 numpy on top of
tests/anim_ref.py, a program interpreter over them, and the programs the pose-graph tests share.

A pose is (T [n, 3], R [n, 4] w x y z, S [n, 3]) in float64. Programs are lists of (op, a, f): a CLIP's `a` is the
position of the clip in rig.clips, a BLEND / ADD's `a` the position of the mask in the `masks` list (or NO_MASK); the
tests translate both into the ids of the implementation they drive. Weights and times are float32 values promoted
exactly, like every other input (see anim_ref).
"""
import numpy as np

import anim_ref

REST, CLIP, BLEND, ADD = 0, 1, 2, 3
NO_MASK = 0xFFFFFFFF
STACK, MAX_OPS = 8, 64

# E_graph_cpu: the shim's float32 interpreter's worst error against this file over graph_rigs() x programs(rig, exact=False), in
# anim_ref.pose_error's metric. Measured 2.812e-5 (rig "chain256", program "depth8"): as for E_cpu, the rounding of 256
# chained float32 products dominates, and the blends in front of them add little (it is below E_cpu's 2.949e-5 because
# these programs sample at other times than the clip tests). Recorded rounded up to two digits;
# tests/test_anim_graph_cpu.py recomputes it and fails above this value; the device bound is 4 x this constant.
E_GRAPH_CPU = 2.9e-5


def f32(x):
    return float(np.float32(x))


def clamp01(x):
    return min(max(x, 0.0), 1.0)


def qmul(p, q):
    return np.array([p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3],
                     p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                     p[0] * q[2] + p[2] * q[0] + p[3] * q[1] - p[1] * q[3],
                     p[0] * q[3] + p[3] * q[0] + p[1] * q[2] - p[2] * q[1]])


def mask_weight(mask, b):
    return 1.0 if mask is None or b >= len(mask) else float(np.float32(mask[b]))


def rest_pose(defaults):
    return (np.array([d[0] for d in defaults], np.float64).reshape(-1, 3),
            np.array([d[1] for d in defaults], np.float64).reshape(-1, 4),
            np.array([d[2] for d in defaults], np.float64).reshape(-1, 3))


def clip_pose(rig, clip, t, defaults):
    T, R, S = (a.copy() for a in rest_pose(defaults))
    t = np.float32(t)
    for ch in clip.channels:
        b = ch["bone"]
        if b < 0 or b >= rig.bones:
            continue
        T[b] = anim_ref.sample_vec(ch.get("T"), t, T[b])
        R[b] = anim_ref.sample_quat(ch.get("R"), t, R[b])
        S[b] = anim_ref.sample_vec(ch.get("S"), t, S[b])
    return T, R, S


def blend(base, target, weight, mask):
    T, R, S = (a.copy() for a in base)
    W = clamp01(f32(weight))
    for b in range(min(len(T), len(target[0]))):
        F = clamp01(W * mask_weight(mask, b))
        T[b] = base[0][b] * (1.0 - F) + target[0][b] * F
        S[b] = base[2][b] * (1.0 - F) + target[2][b] * F
        R[b] = anim_ref.qnormalize(anim_ref.slerp(base[1][b], target[1][b], F))
    return T, R, S


def additive(base, add, weight, mask):
    T, R, S = (a.copy() for a in base)
    for b in range(min(len(T), len(add[0]))):
        F = f32(weight) * mask_weight(mask, b)
        T[b] = base[0][b] + add[0][b] * F
        S[b] = base[2][b] + add[2][b] * F
        R[b] = anim_ref.qnormalize(anim_ref.slerp(base[1][b], qmul(base[1][b], anim_ref.qnormalize(add[1][b])), F))
    return T, R, S


def compose(rig, pose):
    """ComposeSkinningMatrices in float64, [bones, 16]: anim_ref's hierarchy over the pose's local matrices."""
    T, R, S = pose
    return anim_ref.evaluate(rig, None, 0.0, [(T[b], R[b], S[b]) for b in range(rig.bones)])


def well_formed(ops, limits=True):
    depth = 0
    if limits and not 1 <= len(ops) <= MAX_OPS:
        return False
    for op, _, _ in ops:
        if op in (REST, CLIP):
            depth += 1
            if limits and depth > STACK:
                return False
        elif op in (BLEND, ADD):
            if depth < 2:
                return False
            depth -= 1
        else:
            return False
    return depth == 1


def run(rig, ops, masks, defaults):
    """The program's final pose."""
    assert well_formed(ops, limits=False)
    stack = []
    for op, a, f in ops:
        if op == REST:
            stack.append(rest_pose(defaults))
        elif op == CLIP:
            stack.append(clip_pose(rig, rig.clips[a], f, defaults))
        else:
            top = stack.pop()
            mask = None if a == NO_MASK else masks[a]
            stack[-1] = (blend if op == BLEND else additive)(stack[-1], top, f, mask)
    return stack[0]


def evaluate(rig, ops, masks, defaults):
    return compose(rig, run(rig, ops, masks, defaults))


# ---- the shared programs -------------------------------------------------------------------------------------------
def masks_for(rig):
    """Masks of a rig: half weights on the odd bones, one shorter than the skeleton, one longer (weights out of [0, 1]
    included: the blend clamps the product, the additive does not)."""
    n = rig.bones
    rng = np.random.default_rng(100 + n)
    half = np.where(np.arange(n) % 2 == 1, 0.5, 1.0).astype(np.float32)
    short = rng.uniform(0.0, 1.0, max(n // 2, 0)).astype(np.float32)
    long_ = rng.uniform(-0.25, 1.5, n + 3).astype(np.float32)
    return [half, short, long_]


def right_nested(clips, weight):
    """CLIP x depth, then depth - 1 blends: the stack reaches `depth` entries."""
    ops = [(CLIP, c, t) for c, t in clips]
    return ops + [(BLEND, NO_MASK, weight)] * (len(clips) - 1)


def ts_only(clip, name):
    """The clip with its rotation tracks removed: every bone keeps its rest rotation at every time."""
    return anim_ref.Clip(name, clip.duration, [dict(ch, R=None) for ch in clip.channels])


def graph_rig(rig):
    """A view of a shared rig (its arrays, not a copy; the shared rig stays as it is) whose clips are the rig's own
    followed by their translation / scale-only versions: clips 0, 1 = "hold", "slerp", clips 2, 3 = "hold_ts",
    "slerp_ts". A rig without clips stays without."""
    view = anim_ref.Rig("graph_" + rig.name, rig.parents, rig.local_binds, rig.inverse_binds, rig.root_index,
                        rig.source_names)
    view.clips = list(rig.clips) + [ts_only(c, c.name + "_ts") for c in rig.clips]
    return view


_GRAPH_RIGS = None


def graph_rigs():
    global _GRAPH_RIGS
    if _GRAPH_RIGS is None:
        _GRAPH_RIGS = [graph_rig(r) for r in anim_ref.kernel_rigs()] + [
            # 65 bones: a second round of the 64 lanes with one bone in it
            graph_rig(anim_ref.make_rig("chain65", [-1] + list(range(64)), 21)),
            # 130 bones, each the child of the next: the first 128 leave as the palette slice, and all of them have
            # the two bones beyond it among their ancestors
            graph_rig(anim_ref.make_rig("rev130", list(range(1, 130)) + [-1], 22)),
        ]
    return _GRAPH_RIGS


def programs(rig, exact):
    """{name: ops} over a graph_rig's clips and masks_for(rig). exact: only the translation / scale clips and no ADD,
    so that both sides of every blend carry the bone's rest rotation and every slerp takes its linear branch (an
    additive multiplies the rest rotation onto itself, which no longer does).
    An additive adds the whole scale of its pose, weight times (the rest-scale quirk), and a chain multiplies its bones'
    scales up: on rigs of more than four bones the additive weights shrink by 4 / bones, so that a 256-bone chain's
    matrices stay within a few orders of magnitude of 1 and the error metric keeps its meaning."""
    k = min(1.0, 4.0 / rig.bones)
    if not rig.clips:
        progs = {"rest": [(REST, 0, 0.0)],
                 "rest_blend": [(REST, 0, 0.0), (REST, 0, 0.0), (BLEND, 0, 0.5)],
                 "rest_add": [(REST, 0, 0.0), (REST, 0, 0.0), (ADD, 1, f32(0.75 * k))]}
    else:
        ca, cb = (2, 3) if exact else (0, 1)
        ta, tb, tc = 0.2, 0.45, 0.8
        progs = {
            "rest": [(REST, 0, 0.0)],
            "clip": [(CLIP, ca, ta)],
            "blend": [(CLIP, ca, ta), (CLIP, cb, tb), (BLEND, NO_MASK, 0.3)],
            "blend_clamped_hi": [(CLIP, ca, ta), (CLIP, cb, tb), (BLEND, NO_MASK, 1.5)],
            "blend_clamped_lo": [(CLIP, ca, ta), (CLIP, cb, tb), (BLEND, NO_MASK, -1.0)],
            "masked_blend": [(CLIP, ca, ta), (CLIP, cb, tb), (BLEND, 0, 0.5)],
            "long_mask_blend": [(REST, 0, 0.0), (CLIP, cb, tb), (BLEND, 2, 0.9)],
            "additive": [(CLIP, ca, ta), (CLIP, cb, tb), (ADD, NO_MASK, f32(0.4 * k))],
            "additive_unclamped": [(CLIP, ca, ta), (CLIP, cb, tb), (ADD, 1, f32(2.0 * k))],
            # a layer crossfading between two states, over the rest pose
            "crossfade": [(REST, 0, 0.0), (CLIP, ca, ta), (CLIP, cb, tb), (BLEND, NO_MASK, 0.25), (BLEND, NO_MASK, 1.0)],
            # an override layer, then an additive masked layer
            "two_layers": [(REST, 0, 0.0), (CLIP, ca, ta), (CLIP, cb, tc), (BLEND, NO_MASK, 0.6), (BLEND, NO_MASK, 1.0),
                           (CLIP, cb, tb), (ADD, 0, f32(0.35 * k))],
            "depth8": right_nested([(ca if i % 2 == 0 else cb, (ta, tb, tc)[i % 3]) for i in range(STACK)], 0.4),
            "ops63": longest(ca, cb, (ta, tb, tc), additive=not exact, add_weight=f32(0.2 * k)),
        }
    if exact:
        progs = {k: v for k, v in progs.items() if all(op != ADD for op, _, _ in v)}
    return progs


def longest(ca, cb, times, count=MAX_OPS - 1, additive=True, add_weight=0.2):
    """`count` operations (odd: every op pushes one pose or folds two into one, so a program that ends with one entry
    has an odd length, and MAX_OPS - 1 = 63 is the longest the limit admits): a first clip, then rounds of (push,
    combine), every third round (push, push, blend those, combine)."""
    assert count % 2 == 1
    add = ADD if additive else BLEND
    ops = [(CLIP, ca, times[0])]
    i = 0
    while len(ops) < count:
        t = times[i % 3]
        if i % 3 == 2 and count - len(ops) >= 4:
            fold = add if i % 2 else BLEND
            ops += [(CLIP, cb, t), (REST, 0, 0.0), (BLEND, 0, 0.5), (fold, NO_MASK, add_weight if fold == ADD else 0.125)]
        else:
            fold = BLEND if i % 4 else add
            ops += [(CLIP, cb if i % 2 else ca, t), (fold, (NO_MASK, 0, 1, 2)[i % 4], add_weight if fold == ADD else 0.2)]
        i += 1
    return ops
