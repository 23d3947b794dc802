"""k_pose_graph on the device through the library: a one-op program against k_pose (bit for bit), programs whose slerps
all take the linear branch against the shim's float32 interpreter (bit for bit), every other program against the
float64 rules of tests/anim_graph_ref.py, the palette contract and the host-side refusals of tri_pose_graph."""
import ctypes as C

import numpy as np
import pytest

import anim_cases
import anim_graph_cases as cases
import anim_graph_ref as G
import anim_ref
from trident_raster import abi, raster

pytestmark = pytest.mark.gpu

BIND = abi.TRI_POSE_BIND
RIG_NAMES = [r.name for r in G.graph_rigs()]


def _slice(rig):
    return min(rig.bones, abi.TRI_POSE_PALETTE_BONES)


@pytest.fixture(scope="module")
def world():
    """One context and one set with every graph rig: {rig name: (rig, skeleton, clips, masks)}."""
    rigs = {}
    with raster.TriRaster(64, 64, device=0) as ctx, raster.TriAnimSet(0) as aset:
        for rig in G.graph_rigs():
            rigs[rig.name] = (rig,) + cases.device_asset(aset, rig)
        yield ctx, aset, rigs


_CPU, _F64 = {}, {}


def _cpu(rig, name, ops):
    """The shim interpreter's slice for (rig, program), computed once."""
    key = (rig.name, name)
    if key not in _CPU:
        _CPU[key] = cases.cpu_matrices(rig, ops, G.masks_for(rig))[:_slice(rig)]
    return _CPU[key]


def _f64(rig, name, ops):
    key = (rig.name, name)
    if key not in _F64:
        _F64[key] = G.evaluate(rig, ops, G.masks_for(rig), anim_cases.defaults(rig))[:_slice(rig)]
    return _F64[key]


def _run(ctx, aset, rigs, jobs, rng, base=0):
    """jobs: (rig, ops). One tri_pose_graph call with every program in one ops array (behind a few unused records) and
    the slices in a shuffled order with gaps; returns the posed slices, one per job."""
    ops_all = [np.zeros(3, abi.POSE_OP_DTYPE)]
    ops_all[0]["op"] = 99  # never referenced: an op range is checked, not the whole array
    inst, offsets, at, first = [], [0] * len(jobs), base, 3
    for i in rng.permutation(len(jobs)):
        at += int(rng.integers(0, 4))
        offsets[i] = at
        at += _slice(jobs[i][0])
    for (rig, ops), off in zip(jobs, offsets):
        _, sk, clips, masks = rigs[rig.name]
        ops_all.append(cases.device_ops(ops, clips, masks))
        inst.append((sk, first, len(ops), off))
        first += len(ops)
    ctx.pose_graph(aset, inst, np.concatenate(ops_all))
    pal = ctx.read_bone_palette(at)
    return [pal[off:off + _slice(rig)] for (rig, _), off in zip(jobs, offsets)]


def _assert_bits(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} differing words, first at matrix {bad[0][0]} entry {bad[0][1]}: " \
                          f"{got[bad[0][0], bad[0][1]]!r} != {want[bad[0][0], bad[0][1]]!r}"


@pytest.mark.parametrize("name", RIG_NAMES)
def test_one_op_programs_are_k_pose_bit_for_bit(world, name):
    """[CLIP c, t] against tri_pose_palette's (c, t), [REST] against TRI_POSE_BIND: the same words."""
    ctx, aset, rigs = world
    rig, sk, clips, masks = rigs[name]
    plain = [(None, 0.0)] + [(ci, t) for ci in range(len(rig.clips)) for t in (-0.5, 0.0, 0.2, 0.45, 0.5, 0.8, 1.5)]
    n = _slice(rig)
    ctx.pose_palette(aset, [(sk, BIND if ci is None else clips[ci], t, i * (n + 1)) for i, (ci, t) in enumerate(plain)])
    want = ctx.read_bone_palette(len(plain) * (n + 1) - 1)
    ops = [(G.REST, 0, 0.0) if ci is None else (G.CLIP, clips[ci], t) for ci, t in plain]
    ctx.pose_graph(aset, [(sk, i, 1, i * (n + 1)) for i in range(len(plain))], ops)
    got = ctx.read_bone_palette(len(plain) * (n + 1) - 1)
    for i, case in enumerate(plain):
        _assert_bits(got[i * (n + 1):i * (n + 1) + n], want[i * (n + 1):i * (n + 1) + n], f"{name} {case}")


@pytest.mark.parametrize("name", RIG_NAMES)
def test_linear_branch_programs_equal_the_cpu_interpreter(world, name):
    """Translation / scale clips only, no additive: both sides of every blend carry the rest rotation, no sin / acos is
    evaluated, and the palette equals the shim interpreter's matrices as uint32."""
    ctx, aset, rigs = world
    rig = rigs[name][0]
    progs = G.programs(rig, exact=True)
    jobs = [(rig, ops) for ops in progs.values()]
    for got, (pname, ops) in zip(_run(ctx, aset, rigs, jobs, np.random.default_rng(3)), progs.items()):
        _assert_bits(got, _cpu(rig, "exact:" + pname, ops), f"{name} {pname}")


@pytest.mark.parametrize("count", [1, 3, 130])
def test_mixed_skeletons_and_programs_in_one_call(world, count):
    """Instances of every size group with different programs in one call, in a shuffled palette layout."""
    ctx, aset, rigs = world
    pool = [(rigs[n][0], "exact:" + p, ops) for n in RIG_NAMES for p, ops in G.programs(rigs[n][0], exact=True).items()]
    rng = np.random.default_rng(count)
    pick = rng.permutation(len(pool))[:count] if count <= len(pool) else rng.permutation(count) % len(pool)
    jobs = [(pool[i][0], pool[i][2]) for i in pick]
    if count >= 100:
        assert len({abi.TRI_POSE_MAX_BONES if r.bones > 128 else 128 if r.bones > 32 else 32 for r, _ in jobs}) == 3
    for got, i in zip(_run(ctx, aset, rigs, jobs, rng), pick):
        rig, pname, ops = pool[i]
        _assert_bits(got, _cpu(rig, pname, ops), f"{rig.name} {pname}")


@pytest.mark.parametrize("name", RIG_NAMES)
def test_programs_within_four_e_graph_cpu(world, name):
    """Rotating clips, additive layers, depth 8 and the longest program: the error against float64 is at most
    4 x E_graph_cpu, the convention of the clip tests (the device's sinf / acosf are a few ulp where the host's are
    within one; everything else is the interpreter's arithmetic)."""
    ctx, aset, rigs = world
    rig = rigs[name][0]
    progs = G.programs(rig, exact=False)
    jobs = [(rig, ops) for ops in progs.values()]
    worst = (0.0, None)
    for got, (pname, ops) in zip(_run(ctx, aset, rigs, jobs, np.random.default_rng(5)), progs.items()):
        e = anim_ref.pose_error(got, _f64(rig, pname, ops))
        if e > worst[0]:
            worst = (e, pname)
    print(f"device error vs float64, rig {name}: {worst[0]:.4g} at {worst[1]} (bound {4 * G.E_GRAPH_CPU:.4g})")
    assert worst[0] <= 4 * G.E_GRAPH_CPU, worst


def test_uploaded_prefix_then_posed_suffix(world):
    """tri_pose_palette's contract: growing keeps the prefix, instances may not reach into it, a call replaces the
    suffix, count 0 drops it, and so does the next upload."""
    ctx, aset, rigs = world
    prefix = np.arange(5 * 16, dtype=np.float32).reshape(5, 16) + 0.5
    big, small = rigs["graph_chain256"], rigs["graph_chain3"]
    rest = [(G.REST, 0, 0.0)]
    with raster.TriRaster(64, 64, device=0) as c2:
        c2.upload_bone_palette(prefix)
        c2.pose_graph(aset, [(big[1], 0, 1, 7)], rest)  # grows the palette
        pal = c2.read_bone_palette(7 + 128)
        assert np.array_equal(pal[:5], prefix)
        _assert_bits(pal[7:], _cpu(big[0], "rest", rest), "suffix after growth")
        with pytest.raises(raster.TriError) as e:
            c2.pose_graph(aset, [(big[1], 0, 1, 4)], rest)  # inside the prefix
        assert e.value.code == abi.TRI_E_INVALID
        with pytest.raises(raster.TriError):
            c2.read_bone_palette(7 + 129)
        c2.pose_graph(aset, [(small[1], 0, 1, 5)], rest)  # replaces the suffix: the palette is 8 long now
        assert np.array_equal(c2.read_bone_palette(5), prefix)
        _assert_bits(c2.read_bone_palette(8)[5:], _cpu(small[0], "rest", rest), "replaced suffix")
        with pytest.raises(raster.TriError):
            c2.read_bone_palette(9)
        c2.pose_graph(aset, [], [])
        with pytest.raises(raster.TriError):
            c2.read_bone_palette(6)
        assert np.array_equal(c2.read_bone_palette(5), prefix)
        c2.pose_graph(aset, [(small[1], 0, 1, 5)], rest)
        c2.upload_bone_palette(prefix[:2])  # an upload drops the suffix
        with pytest.raises(raster.TriError):
            c2.read_bone_palette(3)
        # the two calls share the palette: a plain-clip call replaces a graph call's suffix and the other way round
        c2.pose_graph(aset, [(small[1], 0, 1, 2)], rest)
        c2.pose_palette(aset, [(small[1], BIND, 0.0, 4)])
        assert np.array_equal(c2.read_bone_palette(2), prefix[:2])
        _assert_bits(c2.read_bone_palette(7)[4:], _cpu(small[0], "rest", rest), "k_pose after k_pose_graph")


def test_calls_queue_without_waiting_and_the_last_one_stands(world):
    """More calls than the staging ring has slots, no synchronisation in between, and both arrays overwritten as soon
    as a call returns."""
    ctx, aset, rigs = world
    rig, sk, clips, masks = rigs["graph_star128"]
    progs = G.programs(rig, exact=True)
    names = (list(progs) * 3)[:10]
    inst = np.zeros(2, abi.POSE_GRAPH_INSTANCE_DTYPE)
    for pname in names:
        ops = np.concatenate([cases.device_ops(progs[pname], clips, masks), cases.device_ops(progs["rest"], clips, masks)])
        inst[0] = (sk, 0, len(progs[pname]), 0)
        inst[1] = (sk, len(progs[pname]), 1, 130)
        ctx.pose_graph(aset, inst, ops)
        inst[:] = (0xFFFFFFF0, 0xFFFFFFF0, 0xFFFFFFF0, 0xFFFFFFF0)  # the call has copied them
        ops[:] = (0xFFFFFFF0, 0xFFFFFFF0, np.nan, 0)
    pal = ctx.read_bone_palette(258)
    _assert_bits(pal[:128], _cpu(rig, "exact:" + names[-1], progs[names[-1]]), "last call")
    _assert_bits(pal[130:], _cpu(rig, "rest", progs["rest"]), "second instance")


def test_ring_wraps_and_regrows_a_used_stage(world):
    """Six calls alternating 1 and 300 instances on a fresh context, behind three single-instance calls that put every
    later call on a stage already used and fenced: 300 instances and their operations are more records than a
    stage's first 512, so the first and the third stage of the ring of four are regrown after use, and the ring wraps
    twice. Every call's palette equals the shim interpreter's, bit for bit."""
    _, aset, rigs = world
    rig = rigs["graph_chain3"][0]
    progs = list(G.programs(rig, exact=True).items())
    rng = np.random.default_rng(11)
    with raster.TriRaster(64, 64, device=0) as c2:
        for count in (1, 1, 1, 1, 300, 1, 300, 1, 300):
            pick = [progs[i % len(progs)] for i in range(count)]
            assert count == 1 or count + sum(len(ops) for _, ops in pick) > 512
            for got, (pname, ops) in zip(_run(c2, aset, rigs, [(rig, ops) for _, ops in pick], rng), pick):
                _assert_bits(got, _cpu(rig, "exact:" + pname, ops), f"{count} instances, {pname}")


def test_refusals_enqueue_nothing(world):
    ctx, aset, rigs = world
    a, b = rigs["graph_chain3"], rigs["graph_forest"]
    sk, ca, ma = a[1], a[2], a[3]
    rest, clip = (G.REST, 0, 0.0), (G.CLIP, ca[0], 0.2)
    blend = (G.BLEND, G.NO_MASK, 0.5)
    ctx.pose_graph(aset, [(sk, 0, 1, 0)], [rest])
    before = ctx.read_bone_palette(3)
    one = lambda ops: ([(sk, 0, len(ops), 0)], ops)  # noqa: E731
    deep = [clip] * 9 + [blend] * 8                  # depth 9
    long_ = [clip] + [clip, blend] * 32              # 65 ops, depth 2
    assert len(long_) == abi.TRI_POSE_MAX_OPS + 1
    bad = [
        one([blend]),                                          # pops an empty stack
        one([rest, blend]),                                    # a blend needs two entries
        one([rest, rest]),                                     # two entries left at the end
        one(deep),
        one(long_),
        ([(sk, 0, 0, 0)], [rest]),                             # no ops
        ([(sk, 1, 1, 0)], [rest]),                             # an op range past the array
        ([(sk, 0xFFFFFFFF, 2, 0)], [rest]),                    # ... whose end wraps in 32 bits
        one([(4, 0, 0.0)]),                                    # unknown op
        one([(G.CLIP, 99999, 0.0)]),                           # unknown clip
        one([(G.CLIP, b[2][0], 0.0)]),                         # a clip of another skeleton
        one([rest, rest, (G.BLEND, 99999, 0.5)]),              # unknown mask
        one([rest, rest, (G.ADD, b[3][0], 0.5)]),              # a mask of another skeleton
        ([(9999, 0, 1, 0)], [rest]),                           # unknown skeleton
        ([(sk, 0, 1, 0), (sk, 0, 1, 2)], [rest]),              # overlap
        ([(sk, 0, 1, abi.TRI_POSE_MAX_PALETTE)], [rest]),      # beyond the palette limit
    ]
    for inst, ops in bad:
        with pytest.raises(raster.TriError) as e:
            ctx.pose_graph(aset, inst, ops)
        assert e.value.code == abi.TRI_E_INVALID, (inst, ops[:3])
    assert np.array_equal(ctx.read_bone_palette(3), before)  # nothing was enqueued
    # the limits themselves pass: depth 8, and 63 ops is the longest well-formed program
    ctx.pose_graph(aset, *one([clip] * 8 + [blend] * 7))
    ctx.pose_graph(aset, *one([clip] + [clip, blend] * 31))
    with pytest.raises(raster.TriError):
        aset.add_mask(9999, [1.0])


def test_set_on_another_device_and_null_arguments(world, hiplib):
    ctx, aset, rigs = world
    inst = np.zeros(1, abi.POSE_GRAPH_INSTANCE_DTYPE)
    inst["op_count"] = 1
    ops = np.zeros(1, abi.POSE_OP_DTYPE)
    assert hiplib.tri_pose_graph(ctx._ctx, None, inst.ctypes.data, 1, ops.ctypes.data, 1) == abi.TRI_E_INVALID
    assert hiplib.tri_pose_graph(ctx._ctx, aset._s, None, 1, ops.ctypes.data, 1) == abi.TRI_E_INVALID
    assert hiplib.tri_pose_graph(ctx._ctx, aset._s, inst.ctypes.data, 1, None, 1) == abi.TRI_E_INVALID
    out = C.c_uint32()
    assert hiplib.tri_animset_add_mask(aset._s, 0, None, 2, C.byref(out)) == abi.TRI_E_INVALID
    assert hiplib.tri_animset_add_mask(aset._s, 0, None, 0, None) == abi.TRI_E_INVALID


def test_group_poses_every_band_or_none(world):
    """tri_group_pose_graph on two bands of one device: a refusal from the check leaves both bands as they were (the
    bands' palettes are not readable through the group; the rendered outcome is the shim tests' subject)."""
    ctx, aset, rigs = world
    rig, sk, clips, masks = rigs["graph_chain3"]
    ops = cases.device_ops(G.programs(rig, exact=False)["two_layers"], clips, masks)
    with raster.TriGroup(64, 64, [0, 0]) as g:
        g.pose_graph([aset], [(sk, 0, len(ops), 0)], ops)
        with pytest.raises(raster.TriError) as e:
            g.pose_graph([aset], [(sk, 0, len(ops) - 1, 0)], ops)
        assert e.value.code == abi.TRI_E_INVALID
        g.pose_graph([aset], [], [])
