"""The shim's CPU animation layer (asset service, channel resolution, the float32 player, the time advance) against the
float64 rules of tests/anim_ref.py, the E_cpu yardstick, and the GPU-free parts of the pose C-ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import anim_cases
import anim_ref
from trident_raster import abi, app

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tri_raster.h")
F = np.float32
FLT_EPSILON = float(np.finfo(np.float32).eps)
IDENT = np.eye(4, dtype=np.float32).reshape(16)
# a float32 product or sum is within 2^-24 relative of exact; the short expressions below chain a handful
TOL = 2e-6


def _rig(name, parents, local_binds=None, inverse_binds=None, root_index=-1, source_names=None):
    n = len(parents)
    lb = np.tile(IDENT, (n, 1)) if local_binds is None else local_binds
    ib = np.tile(IDENT, (n, 1)) if inverse_binds is None else inverse_binds
    return anim_ref.Rig(name, parents, lb, ib, root_index, source_names)


def _both(rig, clip_pos, t):
    """(CPU player, float64 rules) for a rig registered through anim_cases."""
    h, clips = anim_cases.cpu_asset(rig)
    clip = None if clip_pos is None else rig.clips[clip_pos]
    got = app.anim_evaluate(h, None if clip_pos is None else clips[clip_pos], t)
    return got, anim_ref.evaluate(rig, clip, t, anim_cases.defaults(rig))


def _track(times, values):
    return np.array(times, F), np.array(values, F)


# ---- defaults --------------------------------------------------------------------------------------------------------
def test_decompose_matches_the_rules():
    rng = np.random.default_rng(0)
    for _ in range(50):
        q = rng.normal(size=4)
        m = anim_ref.compose(rng.uniform(-2, 2, 3), q / np.linalg.norm(q), rng.uniform(0.2, 3.0, 3)).astype(F)
        t, r, s = app.anim_decompose(m)
        rt, rr, rs = anim_ref.decompose(m)
        assert np.array_equal(t, m[12:15])
        assert np.abs(s - rs).max() <= TOL * rs.max()
        assert np.abs(r - rr).max() <= 4 * TOL
        assert abs(float(np.linalg.norm(r.astype(np.float64))) - 1.0) <= TOL


def test_decompose_leaves_a_zero_length_column_undivided():
    m = anim_ref.compose([1, 2, 3], [1, 0, 0, 0], [2.0, 0.0, 0.5]).astype(F)
    t, r, s = app.anim_decompose(m)
    assert np.array_equal(s, np.array([2.0, 0.0, 0.5], F)) and np.array_equal(t, np.array([1, 2, 3], F))
    assert np.all(np.isfinite(r))
    assert np.abs(r - anim_ref.decompose(m)[1]).max() <= 4 * TOL


# ---- sampling ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_bone():
    rig = _rig("cpu_one", [-1])
    keys = _track([1.0, 2.0, 2.0, 4.0], [[0, 0, 0], [10, 0, 0], [20, 0, 0], [40, 8, 0]])
    rig.clips = [
        anim_ref.Clip("vec", 4.0, [{"bone": 0, "T": keys, "R": None, "S": None}]),
        anim_ref.Clip("single", 1.0, [{"bone": 0, "T": _track([5.0], [[7, 8, 9]]), "R": _track([0.0], [[0, 0, 2, 0]]),
                                       "S": _track([0.0], [[2, 3, 4]])}]),
        # the third key is two ulps (exactly FLT_EPSILON) after the second
        anim_ref.Clip("tiny", 3.0, [{"bone": 0, "T": _track([0.0, 0.5, 0.5 + FLT_EPSILON, 3.0],
                                                             [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]]), "R": None,
                                     "S": None}]),
    ]
    return rig


@pytest.mark.parametrize("t, x, y", [
    (0.0, 0.0, 0.0),       # before the first key: the first key
    (1.0, 0.0, 0.0),       # t <= the first key time
    (1.5, 5.0, 0.0),       # halfway
    (2.0, 20.0, 0.0),      # at a duplicated time: the first interval with t < time[i + 1] is the third, T = 0
    (3.0, 30.0, 4.0),
    (4.0, 40.0, 8.0),      # at the last key: no interval has t < time[i + 1]
    (9.0, 40.0, 8.0),      # after the last key
])
def test_vector_track_known_answers(one_bone, t, x, y):
    got, ref = _both(one_bone, 0, t)
    assert got.shape == (1, 16)
    assert np.array_equal(got[0, 12:15], np.array([x, y, 0], F))
    assert np.abs(got - ref).max() <= TOL * 40


def test_one_ulp_either_side_of_a_key(one_bone):
    below, above = float(np.nextafter(F(2.0), F(0.0))), float(np.nextafter(F(2.0), F(9.0)))
    got, ref = _both(one_bone, 0, below)  # still in [1, 2): just under the second key's 10
    assert 9.99999 < got[0, 12] <= 10.0 and abs(got[0, 12] - ref[0, 12]) <= 40 * TOL
    got, ref = _both(one_bone, 0, above)  # in [2, 4) from the third key's 20
    assert 20.0 <= got[0, 12] < 20.0001 and abs(got[0, 12] - ref[0, 12]) <= 40 * TOL


def test_single_keys_replace_every_track_and_are_normalised(one_bone):
    for t in (-1.0, 0.0, 99.0):
        got, ref = _both(one_bone, 1, t)
        # rotation (0, 0, 2, 0) normalises to a half turn about y; scale 2, 3, 4; translation 7, 8, 9
        want = np.array([-2, 0, 0, 0, 0, 3, 0, 0, 0, 0, -4, 0, 7, 8, 9, 1], F)
        assert np.array_equal(got[0], want)  # (-0 == 0)
        assert np.abs(got - ref).max() == 0


def test_interval_not_longer_than_epsilon_takes_its_first_key(one_bone):
    t = float(np.nextafter(F(0.5), F(1.0)))  # the one float32 inside the interval, halfway
    got, ref = _both(one_bone, 2, t)
    assert got[0, 12] == 1.0 and ref[0, 12] == 1.0  # d <= eps: T = 0, not 0.5


# ---- quaternions -------------------------------------------------------------------------------------------------------
def _rot_clip(name, keys):
    rig = _rig(name, [-1])
    rig.clips = [anim_ref.Clip("r", 1.0, [{"bone": 0, "T": None, "R": keys, "S": None}])]
    return rig


def _rotation_of(m):
    return np.asarray(m, np.float64).reshape(4, 4)[:3, :3]


def test_obtuse_pair_takes_the_short_way():
    h = np.sqrt(0.5)
    rig = _rot_clip("cpu_obtuse", _track([0.0, 1.0], [[1, 0, 0, 0], [-h, 0, 0, -h]]))  # -(quarter turn about z)
    got, ref = _both(rig, 0, 0.5)
    c, s = np.cos(np.pi / 8) ** 2 - np.sin(np.pi / 8) ** 2, 2 * np.sin(np.pi / 8) * np.cos(np.pi / 8)
    want = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]])  # an eighth of a turn about z, columns as rows
    assert np.abs(_rotation_of(got[0]) - want).max() <= 4 * TOL
    assert np.abs(got - ref).max() <= 4 * TOL


def test_nearly_equal_pair_takes_the_linear_branch():
    a = np.array([0.5, 0.5, 0.5, 0.5], F)
    b = (a.astype(np.float64) + [3e-8, -3e-8, 0, 0]).astype(F)
    rig = _rot_clip("cpu_linear", (np.array([0.0, 1.0], F), np.stack([a, b])))
    got, ref = _both(rig, 0, 0.25)
    assert np.all(np.isfinite(got)) and np.abs(got - ref).max() <= 4 * TOL


def test_zero_length_keys():
    rig = _rot_clip("cpu_zero", _track([0.0, 1.0, 2.0], [[0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0]]))
    for t in (0.0, 2.0, 5.0):  # normalize(0) is the identity rotation
        assert np.array_equal(_both(rig, 0, t)[0][0], IDENT)
    got, ref = _both(rig, 0, 0.5)  # slerp(0, x, .5) = sin(pi/4) x, normalised: a half turn about x
    assert np.abs(_rotation_of(got[0]) - np.diag([1, -1, -1])).max() <= 4 * TOL and np.abs(got - ref).max() <= 4 * TOL


# ---- channels -------------------------------------------------------------------------------------------------------------
def test_last_channel_with_keys_wins_per_track():
    rig = _rig("cpu_order", [-1, 0])
    rig.clips = [anim_ref.Clip("c", 1.0, [
        {"bone": 1, "T": _track([0.0], [[1, 1, 1]]), "R": None, "S": _track([0.0], [[2, 2, 2]])},
        {"bone": 1, "T": _track([0.0], [[5, 6, 7]]), "R": None, "S": None},  # replaces T, leaves the earlier S
    ])]
    got, ref = _both(rig, 0, 0.0)
    assert np.array_equal(got[1], np.array([2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, 5, 6, 7, 1], F))
    assert np.abs(got - ref).max() == 0


def test_channel_resolution_by_index_source_name_and_stripped_prefix(capfd):
    names = ["Hips", "mixamorig:Spine", "  Head "]
    rig = _rig("cpu_names", [-1, 0, 1], source_names=names)
    h, _ = anim_cases.cpu_asset(rig)
    key = _track([0.0], [[1, 2, 3]])
    clip = anim_ref.Clip("named", 1.0, [{"bone": 0, "T": key, "R": None, "S": None} for _ in range(6)])
    ch, vt, vv, qt, qv = anim_cases.channel_rows(clip)
    stored = [2, 0, 7, -1, 1, 9]
    source = [None,               # in range, no name: the stored index
              "mixamorig:Spine",  # stored index names another bone: the source-name table
              "Spine",            # out of range: not a source name; the normalised-name table
              "mixamorig:Head",   # trimmed and stripped: "Head" is bone 2's normalised name
              "Spine",            # in range and the bone's normalised name agrees
              "Tail"]             # nothing: skipped with one warning
    ci = app.anim_add_clip(h, clip.name, 1.0, ch, vt, vv, qt, qv, stored_bones=stored, source_names=source)
    capfd.readouterr()
    assert app.anim_resolve_channels(h, ci).tolist() == [2, 1, 1, 2, 1, -1]
    assert capfd.readouterr().err.count("Tail") == 1
    assert app.anim_clip_index(h, "named") == ci and app.anim_clip_index(h, "absent") is None
    pose = app.anim_evaluate(h, ci, 0.0)  # bones 1 and 2 moved, bone 0 not; the stale channel changed nothing
    ref = anim_ref.evaluate(rig, clip, 0.0, anim_cases.defaults(rig), channel_bones=[2, 1, 1, 2, 1, -1])
    assert np.array_equal(pose, ref.astype(F)) and np.array_equal(pose[0], IDENT) and pose[2][12] == 2.0


# ---- hierarchy ------------------------------------------------------------------------------------------------------------
def test_every_shared_rig_matches_the_rules_and_e_cpu_holds():
    """E_cpu: the CPU player's worst error against float64 over the kernel-test rigs, clips and times."""
    worst = (0.0, None)
    for rig in anim_ref.kernel_rigs():
        cases = [(None, 0.0)] + [(ci, t) for ci, clip in enumerate(rig.clips)
                                 for t in anim_ref.sample_times(rig, clip, exact_only=False)]
        for ci, t in cases:
            got, ref = _both(rig, ci, t)
            e = anim_ref.pose_error(got, ref)
            if e > worst[0]:
                worst = (e, (rig.name, ci, t))
    print(f"E_cpu measured {worst[0]:.4g} at {worst[1]}, recorded {anim_ref.E_CPU:.4g}")
    assert worst[0] <= anim_ref.E_CPU, worst
    assert worst[0] >= anim_ref.E_CPU / 4, "E_cpu is recorded far above what is measured: re-record it"


def test_unreached_bones_take_their_local():
    rig = next(r for r in anim_ref.kernel_rigs() if r.name == "forest")
    got, _ = _both(rig, None, 0.0)
    d = anim_cases.defaults(rig)
    for b in (3, 4, 5):  # the second tree is not under root 0: global = local, whatever its parents are
        local = anim_ref.compose(d[b][0], anim_ref.qnormalize(d[b][1]), d[b][2]).reshape(4, 4)
        want = (rig.inverse_binds[b].astype(np.float64).reshape(4, 4) @ local).reshape(16)
        assert np.abs(got[b] - want).max() <= 8 * TOL
    other = next(r for r in anim_ref.kernel_rigs() if r.name == "forest_noroot")
    got, ref = _both(other, None, 0.0)  # without a root both trees are walked: bind pose times inverse bind
    assert np.abs(got - np.tile(IDENT, (6, 1))).max() <= 16 * TOL and np.abs(got - ref).max() <= 16 * TOL


def test_global_that_is_exactly_identity_takes_the_local():
    rig = anim_ref.identity_pair_rig()
    got, ref = _both(rig, None, 0.0)
    # the child's global is translate(1,2,3) * translate(-1,-2,-3) = identity exactly, so it is replaced by the child's
    # local before the inverse bind (scale 2, translate (0, .25, 0)) applies
    assert np.array_equal(got[1], np.array([2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 2, 0, -1, -1.75, -3, 1], F))
    assert np.array_equal(got[0], np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 1.5, 2, 3, 1], F))
    assert np.array_equal(got, ref.astype(F))


def test_fallback_pose_and_refused_cycle(capfd):
    assert np.array_equal(app.anim_evaluate(app.ANIM_NO_HANDLE, None, 0.0), IDENT[None])
    assert np.array_equal(app.anim_evaluate(123456789, 0, 1.0), IDENT[None])
    empty = app.anim_register("test:cpu_empty", [], np.zeros((0, 16)), np.zeros((0, 16)))
    assert np.array_equal(app.anim_evaluate(empty, None, 0.0), IDENT[None])
    loop = _rig("cpu_loop", [1, 0], root_index=0)
    assert anim_ref.evaluate(loop, None, 0.0, anim_cases.defaults(loop)) is None
    capfd.readouterr()
    assert np.array_equal(app.anim_evaluate(anim_cases.cpu_asset(loop)[0], None, 0.0), IDENT[None])
    assert "cycle" in capfd.readouterr().err


def test_registering_an_id_again_keeps_its_handle():
    a = app.anim_register("test:cpu_again", [-1], IDENT[None], IDENT[None])
    moved = anim_ref.compose([4, 5, 6], [1, 0, 0, 0], [1, 1, 1]).astype(F)
    assert app.anim_register("test:cpu_again", [-1, 0], np.stack([IDENT, moved]), np.stack([IDENT, IDENT])) == a
    assert app.anim_evaluate(a, None, 0.0).shape == (2, 16)
    with pytest.raises(app.TriError):
        app.anim_register("", [-1], IDENT[None], IDENT[None])


# ---- the time advance ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def timed():
    rig = _rig("cpu_timed", [-1])
    rig.clips = [anim_ref.Clip("two_seconds", 2.0, [{"bone": 0, "T": _track([0.0, 2.0], [[0, 0, 0], [2, 0, 0]]),
                                                     "R": None, "S": None}])]
    return anim_cases.cpu_asset(rig)


@pytest.mark.parametrize("time, dt, speed, looping, want_time, want_playing", [
    (0.5, 0.25, 1.0, True, 0.75, True),
    (0.5, 0.25, 2.0, True, 1.0, True),       # speed scales the step
    (1.75, 0.5, 1.0, True, 0.25, True),      # forward wrap: fmod(2.25, 2)
    (2.0, 0.0, 1.0, True, 2.0, True),        # exactly the duration is not past it
    (0.25, 0.5, -1.0, True, 1.75, True),     # backward wrap: 2 + fmod(-0.25, 2)
    (1.75, 4.5, 1.0, True, 0.25, True),      # several laps
    (1.75, 0.5, 1.0, False, 2.0, False),     # clamp at the end and stop
    (0.25, 0.5, -1.0, False, 0.0, False),    # clamp at the start and stop
    (0.5, 0.25, 1.0, False, 0.75, True),
])
def test_update_advances_wraps_and_stops(timed, time, dt, speed, looping, want_time, want_playing):
    h, clips = timed
    got = app.anim_advance(h, clips[0], time, dt, speed=speed, looping=looping)
    assert got == (pytest.approx(want_time, abs=1e-6), want_playing)


def test_paused_player_keeps_its_time_and_clipless_player_runs_on(timed):
    h, clips = timed
    assert app.anim_advance(h, clips[0], 0.5, 0.25, playing=False) == (0.5, False)
    assert app.anim_advance(h, None, 1.5, 1.0) == (2.5, True)  # duration 0: no wrap, no stop


# ---- the C-ABI without a GPU ---------------------------------------------------------------------------------------------
def test_pose_struct_layouts_match_the_c_compiler(tmp_path):
    structs = {"tri_pose_bone": abi.TriPoseBone, "tri_pose_channel": abi.TriPoseChannel,
               "tri_pose_instance": abi.TriPoseInstance}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['printf("limits %d %d %u %u %u\\n", TRI_POSE_MAX_BONES, TRI_POSE_PALETTE_BONES, TRI_POSE_BIND, '
              'TRI_POSE_MAX_INSTANCES, TRI_POSE_MAX_PALETTE);', "return 0;}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True,
                                                              check=True).stdout.strip().splitlines()[:-1])
    for cname, py in structs.items():
        assert int(out[f"{cname} size"]) == C.sizeof(py)
        for fname, _ in py._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)
        dt = {"tri_pose_bone": abi.POSE_BONE_DTYPE, "tri_pose_channel": abi.POSE_CHANNEL_DTYPE,
              "tri_pose_instance": abi.POSE_INSTANCE_DTYPE}[cname]
        assert {f: dt.fields[f][1] for f in dt.names} == {f: getattr(py, f).offset for f, _ in py._fields_}
    limits = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True).stdout.strip().splitlines()[-1]
    assert limits.split()[1:] == [str(v) for v in (abi.TRI_POSE_MAX_BONES, abi.TRI_POSE_PALETTE_BONES, abi.TRI_POSE_BIND,
                                                   abi.TRI_POSE_MAX_INSTANCES, abi.TRI_POSE_MAX_PALETTE)]


def test_animset_needs_a_gpu(hiplib):
    """Without a HIP device a set cannot be made: TRI_E_HIP with a message, no CPU stand-in."""
    from tests_gpu_probe import gpu_present

    if gpu_present():
        pytest.skip("a GPU is present")
    s = C.c_void_p()
    assert hiplib.tri_animset_create(-1, C.byref(s)) == abi.TRI_E_HIP
    assert b"device" in hiplib.tri_last_error() and not s.value
    assert hiplib.tri_animset_create(-1, None) == abi.TRI_E_INVALID
    assert hiplib.tri_animset_destroy(None) == abi.TRI_OK
    assert hiplib.tri_pose_palette(None, None, None, 0) == abi.TRI_E_INVALID
    assert hiplib.tri_read_bone_palette(None, None, 0) == abi.TRI_E_INVALID
    assert hiplib.tri_group_pose_palette(None, None, None, 0) == abi.TRI_E_INVALID
    assert hiplib.tri_abi_version() == 2
