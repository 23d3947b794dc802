"""k_pose on the device against the shim's CPU player (bit for bit where no sin / acos is evaluated) and against the
float64 rules of tests/anim_ref.py (interpolated rotations), plus the palette layout and the host-side refusals of
tri_animset_add_* / tri_pose_palette."""
import ctypes as C

import numpy as np
import pytest

import anim_cases
import anim_ref
from trident_raster import abi, app, raster

pytestmark = pytest.mark.gpu

BIND = abi.TRI_POSE_BIND


def _slice(rig):
    return min(rig.bones, abi.TRI_POSE_PALETTE_BONES)


@pytest.fixture(scope="module")
def world():
    """One context, one set with every shared rig: {rig name: (rig, skeleton, clips, cpu handle, cpu clips)}."""
    rigs = {}
    with raster.TriRaster(64, 64, device=0) as ctx, raster.TriAnimSet(0) as aset:
        for rig in anim_ref.kernel_rigs():
            sk, clips = anim_cases.device_asset(aset, rig)
            h, cpu_clips = anim_cases.cpu_asset(rig)
            rigs[rig.name] = (rig, sk, clips, h, cpu_clips)
        yield ctx, aset, rigs


def _layout(cases, rng, base=0):
    """Palette offsets for cases [(rig, ...)] in a shuffled order with gaps: out of order, never overlapping."""
    offsets, at = [0] * len(cases), base
    for i in rng.permutation(len(cases)):
        at += int(rng.integers(0, 4))
        offsets[i] = at
        at += _slice(cases[i][0])
    return offsets, at


def _pose(ctx, aset, rigs, cases, offsets, extent):
    """cases: (rig, clip position in rig.clips or None, time). Returns the posed slices, one per case."""
    inst = []
    for (rig, ci, t), off in zip(cases, offsets):
        _, sk, clips, _, _ = rigs[rig.name]
        inst.append((sk, BIND if ci is None else clips[ci], t, off))
    ctx.pose_palette(aset, inst)
    pal = ctx.read_bone_palette(extent)
    return [pal[off:off + _slice(rig)] for (rig, _, _), off in zip(cases, offsets)]


def _cpu(rigs, rig, ci, t):
    _, _, _, h, cpu_clips = rigs[rig.name]
    return app.anim_evaluate(h, None if ci is None else cpu_clips[ci], t)[:_slice(rig)]


def _exact_cases(rig):
    cases = [(rig, None, 0.0)]
    if rig.clips:
        cases += [(rig, 0, t) for t in anim_ref.sample_times(rig, rig.clips[0], exact_only=True)]
    return cases


def _assert_bits(got, want, what):
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} differing words, first at matrix {bad[0][0]} entry {bad[0][1]}: " \
                          f"{got[bad[0][0], bad[0][1]]!r} != {want[bad[0][0], bad[0][1]]!r}"


@pytest.mark.parametrize("name", [r.name for r in anim_ref.kernel_rigs()])
def test_bit_exact_where_no_library_call_differs(world, name):
    """Bind poses, and the "hold" clip at times where every rotation comes from a single key or an end point while
    translation and scale interpolate: the device palette equals the CPU player's matrices as uint32."""
    ctx, aset, rigs = world
    cases = _exact_cases(rigs[name][0])
    offsets, extent = _layout(cases, np.random.default_rng(11))
    for got, (rig, ci, t) in zip(_pose(ctx, aset, rigs, cases, offsets, extent), cases):
        _assert_bits(got, _cpu(rigs, rig, ci, t), f"{name} clip {ci} t {t!r}")


@pytest.mark.parametrize("count", [1, 3, 130])
def test_bit_exact_mixed_skeletons_in_one_launch(world, count):
    ctx, aset, rigs = world
    pool = [c for name in rigs for c in _exact_cases(rigs[name][0])]
    rng = np.random.default_rng(count)
    cases = [pool[i] for i in rng.permutation(len(pool))[:count]] if count <= len(pool) else \
        [pool[i % len(pool)] for i in rng.permutation(count)]
    offsets, extent = _layout(cases, rng)
    want = {}
    for got, case in zip(_pose(ctx, aset, rigs, cases, offsets, extent), cases):
        key = (case[0].name, case[1], case[2])
        if key not in want:
            want[key] = _cpu(rigs, *case)
        _assert_bits(got, want[key], f"{key}")


@pytest.mark.parametrize("name", [r.name for r in anim_ref.kernel_rigs() if r.clips])
def test_interpolated_rotations_within_four_e_cpu(world, name):
    """Slerp between distinct keys: the error against float64 is at most 4 x E_cpu (the device's sinf / acosf are a
    few ulp where the host's are within one; everything else is the CPU player's arithmetic)."""
    ctx, aset, rigs = world
    rig = rigs[name][0]
    cases = [(rig, ci, t) for ci, clip in enumerate(rig.clips) for t in anim_ref.sample_times(rig, clip, exact_only=False)]
    offsets, extent = _layout(cases, np.random.default_rng(5))
    d = anim_cases.defaults(rig)
    worst = (0.0, None)
    for got, (_, ci, t) in zip(_pose(ctx, aset, rigs, cases, offsets, extent), cases):
        ref = anim_ref.evaluate(rig, rig.clips[ci], t, d)[:_slice(rig)]
        e = anim_ref.pose_error(got, ref)
        if e > worst[0]:
            worst = (e, (rig.clips[ci].name, t))
    print(f"device error vs float64, rig {name}: {worst[0]:.4g} at {worst[1]} (bound {4 * anim_ref.E_CPU:.4g})")
    assert worst[0] <= 4 * anim_ref.E_CPU, worst


def test_uploaded_prefix_then_posed_suffix(world):
    """The palette is the uploaded prefix followed by the posed suffix: growing keeps the prefix, instances may not
    reach into it, count 0 drops the suffix, the next upload drops it too."""
    ctx, aset, rigs = world
    prefix = np.arange(5 * 16, dtype=np.float32).reshape(5, 16) + 0.5
    with raster.TriRaster(64, 64, device=0) as c2:
        c2.upload_bone_palette(prefix)
        rig, sk, clips, h, cpu_clips = rigs["chain256"]
        c2.pose_palette(aset, [(sk, BIND, 0.0, 7)])  # grows the palette
        pal = c2.read_bone_palette(7 + 128)
        assert np.array_equal(pal[:5], prefix)
        _assert_bits(pal[7:], app.anim_evaluate(h, None, 0.0)[:128], "suffix after growth")
        with pytest.raises(raster.TriError):
            c2.pose_palette(aset, [(sk, BIND, 0.0, 4)])  # inside the prefix
        with pytest.raises(raster.TriError):
            c2.read_bone_palette(7 + 129)
        small = rigs["chain3"]
        c2.pose_palette(aset, [(small[1], small[2][0], 0.25, 5)])  # replaces the suffix: the palette is 8 long now
        assert np.array_equal(c2.read_bone_palette(5), prefix)
        _assert_bits(c2.read_bone_palette(8)[5:], app.anim_evaluate(small[3], small[4][0], 0.25), "replaced suffix")
        with pytest.raises(raster.TriError):
            c2.read_bone_palette(9)
        c2.pose_palette(aset, [])
        with pytest.raises(raster.TriError):
            c2.read_bone_palette(6)
        assert np.array_equal(c2.read_bone_palette(5), prefix)
        c2.pose_palette(aset, [(small[1], BIND, 0.0, 5)])
        c2.upload_bone_palette(prefix[:2])  # an upload drops the suffix
        with pytest.raises(raster.TriError):
            c2.read_bone_palette(3)


def test_calls_queue_without_waiting_and_the_last_one_stands(world):
    """More calls than the staging ring has slots, no synchronisation in between: each replaces the suffix in stream
    order, and the records may be overwritten as soon as a call returns."""
    ctx, aset, rigs = world
    rig, sk, clips, h, cpu_clips = rigs["star128"]
    inst = np.zeros(2, abi.POSE_INSTANCE_DTYPE)
    times = [0.0, 0.1, 0.2, 0.3, 0.7, 0.8, 0.9, 0.05, 0.15, 0.95]
    for t in times:
        inst[0] = (sk, clips[0], t, 0)
        inst[1] = (sk, BIND, 0.0, 130)
        ctx.pose_palette(aset, inst)
        inst[:] = (0xFFFFFFF0, 0xFFFFFFF0, np.nan, 0xFFFFFFF0)  # the call has copied them
    pal = ctx.read_bone_palette(258)
    _assert_bits(pal[:128], app.anim_evaluate(h, cpu_clips[0], times[-1]), "last call")
    _assert_bits(pal[130:], app.anim_evaluate(h, None, 0.0), "second instance")


def test_pose_palette_refuses_bad_instances(world):
    ctx, aset, rigs = world
    a, b = rigs["chain3"], rigs["forest"]
    ctx.pose_palette(aset, [(a[1], BIND, 0.0, 0)])
    before = ctx.read_bone_palette(3)
    for bad in ([(9999, BIND, 0.0, 0)],                          # unknown skeleton
                [(a[1], 9999, 0.0, 0)],                          # unknown clip
                [(a[1], b[2][0], 0.0, 0)],                       # a clip of another skeleton
                [(a[1], BIND, 0.0, 0), (a[1], BIND, 0.0, 2)],    # overlap
                [(a[1], BIND, 0.0, abi.TRI_POSE_MAX_PALETTE)]):  # beyond the palette limit
        with pytest.raises(raster.TriError) as e:
            ctx.pose_palette(aset, bad)
        assert e.value.code == abi.TRI_E_INVALID
    assert np.array_equal(ctx.read_bone_palette(3), before)  # nothing was enqueued


def test_animset_refuses_bad_skeletons_and_clips(world):
    ctx, aset, rigs = world

    def bones(parents):
        b = np.zeros(len(parents), abi.POSE_BONE_DTYPE)
        b["parent"] = parents
        b["rotation"][:, 0] = 1.0
        b["scale"][:, :3] = 1.0
        b["inverse_bind"] = np.eye(4, dtype=np.float32).reshape(16)
        return b

    for parents, root in (([], -1), ([-1] * 257, -1), ([-1, 2], -1), ([1, 0], 0), ([0], -1), ([2, 0, 1], -1)):
        with pytest.raises(raster.TriError) as e:
            aset.add_skeleton(bones(parents), root)
        assert e.value.code == abi.TRI_E_INVALID, parents
    # a loop the traversal never reaches is no obstacle: bones 1 and 2 take global = local
    sk = aset.add_skeleton(bones([-1, 2, 1]), -1)
    ch = np.zeros(1, abi.POSE_CHANNEL_DTYPE)
    vals = np.zeros((3, 3), np.float32)

    def clip(bone=0, first=0, count=3, times=(0.0, 0.5, 1.0), duration=1.0):
        ch[0] = (bone, first, count, 0, 0, 0, 0, 0)
        return aset.add_clip(sk, ch, np.array(times, np.float32), vals, [], np.zeros((0, 4)), duration)

    clip()
    for kw in (dict(bone=3), dict(first=1), dict(times=(0.0, 0.6, 0.5)), dict(times=(0.0, np.nan, 1.0)),
               dict(times=(0.0, np.inf, np.inf)), dict(duration=np.nan)):
        with pytest.raises(raster.TriError) as e:
            clip(**kw)
        assert e.value.code == abi.TRI_E_INVALID, kw
    with pytest.raises(raster.TriError):
        aset.add_clip(9999, ch, [0, 0, 0], vals, [], np.zeros((0, 4)), 1.0)
    # a refused add leaves the set usable
    ctx.pose_palette(aset, [(sk, BIND, 0.0, 0)])
    assert np.array_equal(ctx.read_bone_palette(3), np.tile(np.eye(4, dtype=np.float32).reshape(16), (3, 1)))


def test_set_on_another_device_and_null_arguments(world, hiplib):
    ctx, aset, rigs = world
    inst = np.zeros(1, abi.POSE_INSTANCE_DTYPE)
    assert hiplib.tri_pose_palette(None, aset._s, inst.ctypes.data, 1) == abi.TRI_E_INVALID
    assert hiplib.tri_pose_palette(ctx._ctx, None, inst.ctypes.data, 1) == abi.TRI_E_INVALID
    assert hiplib.tri_pose_palette(ctx._ctx, aset._s, None, 1) == abi.TRI_E_INVALID
    assert hiplib.tri_animset_destroy(None) == abi.TRI_OK
    assert hiplib.tri_animset_create(0, None) == abi.TRI_E_INVALID
    s = C.c_void_p()
    assert hiplib.tri_animset_create(4096, C.byref(s)) == abi.TRI_E_INVALID and not s.value
