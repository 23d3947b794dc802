"""The pose-space rules (include/tri_raster.h, "Pose space") on the CPU: known answers worked out by hand against both
the float64 restatement (tests/anim_graph_ref.py) and the shim's float32 interpreter, and the interpreter's measured
error against float64 over the shared programs."""
import numpy as np
import pytest

import anim_cases
import anim_graph_cases as cases
import anim_graph_ref as G
import anim_ref
from trident_raster import abi, app, raster

A = float(np.sqrt(0.5))


def _translate(t):
    return anim_ref.compose(t, [1, 0, 0, 0], [1, 1, 1]).astype(np.float32)


def _const(bone, T=None, R=None, S=None):
    key = lambda v: None if v is None else (np.array([0.0], np.float32), np.array([v], np.float32))  # noqa: E731
    return {"bone": bone, "T": key(T), "R": key(R), "S": key(S)}


@pytest.fixture(scope="module")
def kat():
    """Two parentless bones with identity inverse binds, so a pose matrix is the bone's local matrix: the rest pose is
    T = (0.5, 0, 0) / (0, 0.25, 0), identity rotation, scale 1. Clips of single keys: "a" and "b" move and scale both
    bones, "rx" / "ry" turn bone 0 a quarter about x / y."""
    rig = anim_ref.Rig("graph_kat", [-1, -1], np.stack([_translate([0.5, 0, 0]), _translate([0, 0.25, 0])]),
                       np.stack([_translate([0, 0, 0])] * 2))
    rig.clips = [
        anim_ref.Clip("a", 1.0, [_const(0, T=[1, 2, 3], S=[2, 2, 2]), _const(1, T=[4, 0, 0])]),
        anim_ref.Clip("b", 1.0, [_const(0, T=[3, 2, 1], S=[4, 1, 1]), _const(1, T=[0, 8, 0], S=[1, 3, 1])]),
        anim_ref.Clip("rx", 1.0, [_const(0, R=[A, A, 0, 0])]),
        anim_ref.Clip("ry", 1.0, [_const(0, R=[A, 0, A, 0])]),
    ]
    return rig


def _both(rig, ops, masks=()):
    """The program's matrices from float64 and from the shim, as [bones, 4, 4] indexed [bone][column][row]."""
    d = anim_cases.defaults(rig)
    ref = G.evaluate(rig, ops, list(masks), d).reshape(-1, 4, 4)
    got = cases.cpu_matrices(rig, ops, list(masks)).astype(np.float64).reshape(-1, 4, 4)
    return ref, got


def _expect(rig, ops, masks, T, S=None, rot=None):
    """Both implementations give translation T[b], scale S[b] (default 1) times the rotation columns rot (default I)."""
    for name, m in zip(("float64", "shim"), _both(rig, ops, masks)):
        for b in range(rig.bones):
            s = [1, 1, 1] if S is None else S[b]
            r = np.eye(3) if rot is None or rot[b] is None else np.asarray(rot[b], np.float64)
            want = np.zeros((4, 4))
            for j in range(3):
                want[j][:3] = r[j] * s[j]
            want[3] = [T[b][0], T[b][1], T[b][2], 1.0]
            assert np.allclose(m[b], want, rtol=0, atol=2e-6), (name, b, m[b], want)


AB = [(G.CLIP, 0, 0.0), (G.CLIP, 1, 0.0)]


def test_blend_at_zero_one_and_half_with_a_half_mask(kat):
    _expect(kat, AB + [(G.BLEND, G.NO_MASK, 0.0)], [], T=[[1, 2, 3], [4, 0, 0]], S=[[2, 2, 2], [1, 1, 1]])
    _expect(kat, AB + [(G.BLEND, G.NO_MASK, 1.0)], [], T=[[3, 2, 1], [0, 8, 0]], S=[[4, 1, 1], [1, 3, 1]])
    # bone 0 at F = 0.5, bone 1 at F = 0.5 * 0.5
    _expect(kat, AB + [(G.BLEND, 0, 0.5)], [[1.0, 0.5]], T=[[2, 2, 2], [3, 2, 0]], S=[[3, 1.5, 1.5], [1, 1.5, 1]])


def test_blend_weight_clamps(kat):
    _expect(kat, AB + [(G.BLEND, G.NO_MASK, 1.5)], [], T=[[3, 2, 1], [0, 8, 0]], S=[[4, 1, 1], [1, 3, 1]])
    _expect(kat, AB + [(G.BLEND, G.NO_MASK, -1.0)], [], T=[[1, 2, 3], [4, 0, 0]], S=[[2, 2, 2], [1, 1, 1]])
    # the product with the mask is clamped too: 1.0 * 3.0 -> 1, 1.0 * -2.0 -> 0
    _expect(kat, AB + [(G.BLEND, 0, 1.0)], [[3.0, -2.0]], T=[[3, 2, 1], [4, 0, 0]], S=[[4, 1, 1], [1, 1, 1]])


def test_additive_is_unclamped_and_adds_rest_scales(kat):
    # weight 2: a + 2 * b, scales included
    _expect(kat, AB + [(G.ADD, G.NO_MASK, 2.0)], [], T=[[7, 6, 5], [4, 16, 0]], S=[[10, 4, 4], [3, 7, 3]])
    # an additive rest pose adds its translation and its unit scale: the quirk kept
    _expect(kat, [(G.CLIP, 0, 0.0), (G.REST, 0, 0.0), (G.ADD, G.NO_MASK, 1.0)], [], T=[[1.5, 2, 3], [4, 0.25, 0]],
            S=[[3, 3, 3], [2, 2, 2]])
    # a negative product with the mask subtracts
    _expect(kat, AB + [(G.ADD, 0, 1.0)], [[-1.0, 0.5]], T=[[-2, 0, 2], [4, 4, 0]], S=[[-2, 1, 1], [1.5, 2.5, 1.5]])


def test_quaternion_product_by_hand(kat):
    # (a, a, 0, 0) * (a, 0, a, 0) with a = sqrt(1/2) is (1/2, 1/2, 1/2, 1/2): x -> y -> z -> x
    assert np.allclose(G.qmul([A, A, 0, 0], [A, 0, A, 0]), [0.5, 0.5, 0.5, 0.5], rtol=0, atol=1e-15)
    assert np.allclose(G.qmul([A, 0, A, 0], [A, A, 0, 0]), [0.5, 0.5, 0.5, -0.5], rtol=0, atol=1e-15)
    cyc = [[0, 1, 0], [0, 0, 1], [1, 0, 0]]  # columns of the rotation of (1/2, 1/2, 1/2, 1/2)
    # additive at F = 1: slerp(base, base * add, 1) = base * add (scale 1 + 1 = 2 on every bone: the quirk)
    _expect(kat, [(G.CLIP, 2, 0.0), (G.CLIP, 3, 0.0), (G.ADD, G.NO_MASK, 1.0)], [], T=[[1, 0, 0], [0, 0.5, 0]],
            S=[[2, 2, 2], [2, 2, 2]], rot=[cyc, None])
    # the other order turns the other way round z
    other = anim_ref.to_mat3_columns(np.array([0.5, 0.5, 0.5, -0.5]))
    _expect(kat, [(G.CLIP, 3, 0.0), (G.CLIP, 2, 0.0), (G.ADD, G.NO_MASK, 1.0)], [], T=[[1, 0, 0], [0, 0.5, 0]],
            S=[[2, 2, 2], [2, 2, 2]], rot=[other, None])


def test_mask_shorter_than_the_skeleton(kat):
    # one weight for two bones: bone 0 keeps the base, bone 1 weighs 1.0
    _expect(kat, AB + [(G.BLEND, 0, 0.5)], [[0.0]], T=[[1, 2, 3], [2, 4, 0]], S=[[2, 2, 2], [1, 2, 1]])
    # an empty mask weighs 1.0 everywhere; surplus weights are dropped
    _expect(kat, AB + [(G.BLEND, 0, 0.5)], [[]], T=[[2, 2, 2], [2, 4, 0]], S=[[3, 1.5, 1.5], [1, 2, 1]])
    _expect(kat, AB + [(G.BLEND, 0, 0.5)], [[1.0, 1.0, 0.0, 0.0]], T=[[2, 2, 2], [2, 4, 0]], S=[[3, 1.5, 1.5], [1, 2, 1]])


@pytest.mark.parametrize("rig", G.graph_rigs(), ids=lambda r: r.name)
def test_one_clip_program_is_the_player(rig):
    """[CLIP] and [REST] are the CPU player's clip and bind poses bit for bit: the same code below the pose."""
    h, cpu_clips = anim_cases.cpu_asset(rig)
    assert np.array_equal(cases.cpu_matrices(rig, [(G.REST, 0, 0.0)], []).view(np.uint32),
                          app.anim_evaluate(h, None, 0.0).view(np.uint32))
    for ci in range(len(rig.clips)):
        for t in (0.0, 0.2, 0.5, 1.5):
            assert np.array_equal(cases.cpu_matrices(rig, [(G.CLIP, ci, t)], []).view(np.uint32),
                                  app.anim_evaluate(h, cpu_clips[ci], t).view(np.uint32)), (ci, t)


def test_interpreter_error_against_float64_is_within_the_recorded_value():
    """E_graph_cpu: recomputed over every graph rig x its programs, and not above what anim_graph_ref records."""
    worst = (0.0, None)
    for rig in G.graph_rigs():
        d = anim_cases.defaults(rig)
        masks = G.masks_for(rig)
        for name, ops in G.programs(rig, exact=False).items():
            assert G.well_formed(ops), name
            e = anim_ref.pose_error(cases.cpu_matrices(rig, ops, masks), G.evaluate(rig, ops, masks, d))
            if e > worst[0]:
                worst = (e, (rig.name, name))
    print(f"E_graph_cpu measured {worst[0]:.4g} at {worst[1]} (recorded {G.E_GRAPH_CPU:.4g})")
    assert worst[0] <= G.E_GRAPH_CPU, worst
    assert worst[0] > 0.25 * G.E_GRAPH_CPU, "the recorded value no longer describes the interpreter"


def test_exact_programs_hold_no_additive_and_the_longest_has_63_ops():
    for rig in G.graph_rigs():
        for exact in (False, True):
            for name, ops in G.programs(rig, exact).items():
                assert G.well_formed(ops), (rig.name, name)
                assert not exact or all(op != G.ADD for op, _, _ in ops)
        if rig.clips:
            progs = G.programs(rig, False)
            assert len(progs["ops63"]) == abi.TRI_POSE_MAX_OPS - 1
            depth = peak = 0
            for op, _, _ in progs["depth8"]:
                depth += 1 if op in (G.REST, G.CLIP) else -1
                peak = max(peak, depth)
            assert peak == abi.TRI_POSE_STACK


def test_interpreter_refuses_bad_programs(kat):
    h, clips = anim_cases.cpu_asset(kat)
    for bad, masks in (([], []),                                                        # no pose left
                       ([(G.BLEND, G.NO_MASK, 0.5)], []),                               # pops an empty stack
                       ([(G.REST, 0, 0.0), (G.BLEND, G.NO_MASK, 0.5)], []),             # needs two
                       ([(G.REST, 0, 0.0), (G.REST, 0, 0.0)], []),                      # two left
                       ([(7, 0, 0.0)], []),                                             # unknown op
                       ([(G.CLIP, 99, 0.0)], []),                                       # unknown clip
                       ([(G.REST, 0, 0.0), (G.REST, 0, 0.0), (G.BLEND, 0, 0.5)], [])):  # unknown mask
        with pytest.raises(raster.TriError) as e:
            app.anim_eval_program(h, bad, masks)
        assert e.value.code == abi.TRI_E_INVALID, bad
    with pytest.raises(raster.TriError):
        app.anim_eval_program(0xDEAD, [(G.REST, 0, 0.0)], [])
    # the CPU interpreter has no depth or length limit: the device's are FitsDevice's business
    deep = G.right_nested([(0, 0.0)] * 12, 0.5)
    assert app.anim_eval_program(h, deep, []).shape == (2, 16)
