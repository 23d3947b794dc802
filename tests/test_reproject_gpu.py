"""GPU tests of the history reprojection pass (include/tri_raster.h "history reprojection"): k_reproject, tri_history
and its place behind the frame.

The bar throughout: the device's warped colour and mask == tests/reproject_ref.py's float32 restatement, fed with the
device's own colour, ids and depth of both frames and the library's table (tri_motion_matrices), compared as bytes —
ZERO mismatches: the rule fixes every operation. The cases are the smallest at which the kernel can go wrong: 100 x 70
(1750 whole vectors, mixed waves), 101 x 70 (rows that are not 16-B aligned, vectors that straddle a row end, a two-pixel
tail), 37 x 23 under caller-bound targets at a 4-B offset (one pixel per lane), one draw (the wave-uniform lookup), 1024
draws of 2 x 2 px (every lane gathers another table row).
"""
import ctypes as C

import numpy as np
import pytest

import id_ref
import motion_ref as mr
import reproject_ref as rr
import scene_cases as sc
from test_reproject_cpu import quad_split, two_quads, two_quads_history

pytestmark = pytest.mark.gpu
F = np.float32


def open_raster(scene, **kw):
    """A context with the scene loaded and the id and motion outputs on."""
    from trident_raster import raster, scenes

    r = raster.TriRaster(scene.width, scene.height, **kw)
    scenes.load_scene(r, scene)
    r.set_id_output(True)
    r.set_motion_output(True)
    return r


def render(r, scene, hist):
    """One frame of `scene` (same geometry as the loaded one) under the motion history `hist` (None: none)."""
    r.set_frame(scene.ubo, scene.clear)
    r.set_draws(scene.draws)
    if hist is None:
        r.set_motion_history(None)
    else:
        r.set_motion_history(*hist)
    r.render_frame()


def snapshot(r):
    """(ids, depth bits, colour) of the context's last frame."""
    col, dep = r.readback()
    return r.read_ids(), dep, col


def check(tag, r, h, scene, hist, prev, tolerance=0.0):
    """The object's outputs against the restatement over the device's own frames; returns (current frame, warped,
    mask): the frame is the next call's `prev`."""
    from trident_raster import raster

    cur = snapshot(r)
    got_c, got_m = h.read()
    table = raster.motion_matrices(scene.ubo, scene.draws, hist)
    want_c, want_m = rr.restate(table, cur[0], cur[1], cur[2], prev, scene.width, scene.height, tolerance)
    bad_m = int((got_m != want_m).sum())
    bad_c = int((got_c != want_c).any(axis=-1).sum())
    counts = {k: int((want_m == v).sum()) for k, v in (("valid", 0), ("none", 1), ("no_proj", 2), ("outside", 4), ("id", 8), ("depth", 16))}
    print(f"REPROJECT {tag}: {scene.width} x {scene.height}, {counts}, mask mismatches {bad_m}, colour mismatches {bad_c}")
    assert got_m.shape == want_m.shape and got_c.shape == want_c.shape
    assert bad_m == 0, f"{tag}: {bad_m} mask mismatches"
    assert bad_c == 0, f"{tag}: {bad_c} colour mismatches"
    return cur, got_c, got_m


def two_frames(tag, s, hist, tolerance=0.0, **kw):
    """The previous frame, then `s`, on one context and one object; returns what check() returns for the second."""
    from trident_raster import raster

    was = rr.previous_scene(s, hist)
    with open_raster(s, **kw) as r, raster.TriHistory(s.width, s.height) as h:
        render(r, was, None)
        h.reproject(r)
        prev, c0, m0 = check(tag + " / first", r, h, was, None, None)
        assert (m0 == rr.NO_HISTORY).all() and np.array_equal(c0, prev[2])  # first pass: 1 everywhere, the current colour
        render(r, s, hist)
        h.reproject(r, tolerance)
        return check(tag, r, h, s, hist, prev, tolerance)


def chain():
    """Three consecutive frames of the cubes and the quad: [(scene, history)], the first without history."""
    s2 = id_ref.cubes_and_quad()
    h2 = mr.previous_frame(s2)
    s1 = rr.previous_scene(s2, h2)
    h1 = mr.previous_frame(s1, camera_move=mr.rigid((-0.05, 0.04, 0.1), (0.5, 1.5, -0.4)))
    s0 = rr.previous_scene(s1, h1)
    return [(s0, None), (s1, h1), (s2, h2)]


# ---- k_reproject ----------------------------------------------------------------------------------------------------
def test_three_moved_draws():
    s = id_ref.cubes_and_quad()
    _, _, m = two_frames(s.name, s, mr.previous_frame(s))
    assert (m == 0).any() and (m == rr.OUTSIDE).any() and (m == rr.ID).any()


def test_a_width_of_101():
    """Rows of 404 B, vectors that straddle row ends, and an image that ends in a partial vector."""
    s = id_ref.cubes_and_quad(101, 70)
    assert (s.width * s.height) % 4 == 2
    _, _, m = two_frames(s.name + "_101", s, mr.previous_frame(s))
    assert (m == 0).any() and (m == rr.OUTSIDE).any() and (m == rr.ID).any()


def test_caller_bound_targets_at_a_4_byte_offset():
    """37 x 23 rendered into a caller's colour and depth that start 4 B past a 16-B boundary: one pixel per lane."""
    import torch

    from trident_raster import raster

    s = id_ref.cubes_and_quad(37, 23)
    hist = mr.previous_frame(s)
    was = rr.previous_scene(s, hist)
    n = s.width * s.height
    col = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
    dep = torch.zeros(n + 1, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert col[1:].data_ptr() % 16 == 4 and dep[1:].data_ptr() % 16 == 4
    with open_raster(s) as r, raster.TriHistory(s.width, s.height) as h:
        r.bind_output(col[1:].data_ptr(), dep[1:].data_ptr())
        render(r, was, None)
        h.reproject(r)
        prev, _, m0 = check("bound / first", r, h, was, None, None)
        assert (m0 == rr.NO_HISTORY).all()
        render(r, s, hist)
        h.reproject(r)
        cur, _, m = check("bound", r, h, s, hist, prev)
        assert (m == 0).any() and (m != 0).any()
        r.synchronize()
        assert np.array_equal(col[1:].cpu().numpy().view(np.uint8).reshape(s.height, s.width, 4), cur[2])  # (it was the caller's)
        r.bind_output(None, None)


def test_one_draw():
    """A single-draw frame: whole waves under one id take the wave-uniform lookup, others the gather."""
    from trident_raster import scenes

    s = scenes.scene_c1_cube(1, 100, 70, skybox="solid")
    s.name = "reproject_c1_cube"
    cur, _, m = two_frames(s.name, s, mr.previous_frame(s))
    waves = cur[0].reshape(-1)[: cur[0].size // 256 * 256].reshape(-1, 256)  # a wave's 64 lanes x 4 pixels
    uniform = (waves == waves[:, :1]).all(axis=1)
    assert uniform.any() and not uniform.all() and (m == 0).any()


def test_1024_small_draws():
    """64 x 64 covered by 1024 quads of 2 x 2 px, each its own draw with its own whole-pixel translation one frame ago."""
    w = h = 64
    rects = [(2 * i, 2 * j, 2 * i + 2, 2 * j + 2, 0.25 + 0.5 * ((i * 7 + j * 3) % 16) / 16.0) for j in range(32) for i in range(32)]
    s = id_ref.pixel_quads("reproject_1024_quads", w, h, rects)
    v, p = mr.camera_of(s.ubo)
    shifts = [((k * 5) % 13 - 6, (k * 11) % 9 - 4) for k in range(1024)]
    prev = np.array([mr.to_cm(mr.rigid((tx, ty, 0.0))).reshape(16) for tx, ty in shifts], F)
    cur, _, m = two_frames(s.name, s, (v, p, prev))
    assert len(np.unique(cur[0])) == 1024 and (m == 0).any() and (m == rr.ID).any()


def test_a_previous_camera_turned_round():
    """Every point lay behind the previous camera: mask 2 everywhere, the warped image is the current one."""
    s = id_ref.cubes_and_quad()
    hist = mr.previous_frame(s, camera_move=mr.rigid((0, 0, 0), (0.0, 180.0, 0.0)))
    cur, c, m = two_frames("turned", s, hist)
    assert (m == rr.NO_PROJ).all() and np.array_equal(c, cur[2])


def test_first_pass_and_after_a_reset():
    from trident_raster import raster

    s = id_ref.cubes_and_quad()
    still = (*mr.camera_of(s.ubo), None)
    with open_raster(s) as r, raster.TriHistory(s.width, s.height) as h:
        render(r, s, still)
        h.reproject(r)
        prev, c, m = check("first", r, h, s, still, None)
        assert (m == rr.NO_HISTORY).all() and np.array_equal(c, prev[2])
        h.reproject(r)
        _, c, m = check("second", r, h, s, still, prev)
        assert (m == 0).all()
        h.reset()
        h.reproject(r)
        _, c, m = check("after the reset", r, h, s, still, None)
        assert (m == rr.NO_HISTORY).all() and np.array_equal(c, prev[2])
        h.reproject(r)
        _, _, m = check("and the one after", r, h, s, still, prev)
        assert (m == 0).all()


def test_a_still_scene():
    """Nothing moved: mask 0 everywhere, warped == the previous frame == the current frame."""
    s = id_ref.cubes_and_quad()
    cur, c, m = two_frames("still", s, (*mr.camera_of(s.ubo), None))
    assert (m == 0).all() and np.array_equal(c, cur[2])


def test_a_quad_moved_aside_uncovers_the_background():
    w, h = 64, 48
    s = id_ref.pixel_quads("reproject_moved_quad", w, h, [(10, 8, 34, 40, 0.5)])
    v, p = mr.camera_of(s.ubo)
    prev = np.array([mr.to_cm(mr.rigid((20.0, 0.0, 0.0))).reshape(16)], F)  # it stood 20 px to the right
    cur, _, m = two_frames(s.name, s, (v, p, prev))
    uncovered = np.zeros((h, w), bool)
    uncovered[8:40, 34:54] = True  # background now, the quad one frame ago
    assert (m[uncovered] == rr.ID).all() and (m == rr.ID).sum() == uncovered.sum()
    assert (m[cur[0] == 1] == 0).all()


def test_depth_bit_between_two_quads_of_one_id():
    from trident_raster import raster

    s = two_quads()
    hist = two_quads_history(s)
    was = rr.previous_scene(s, hist)
    with open_raster(s) as r, raster.TriHistory(s.width, s.height) as h:
        render(r, was, None)
        h.reproject(r)
        prev = snapshot(r)
        render(r, s, hist)
        cur = snapshot(r)
        tol = 0.25 * min(quad_split(cur[1], cur[0])[1], quad_split(prev[1], prev[0])[1])
        h.reproject(r, tol)
        _, _, m = check("two quads", r, h, s, hist, prev, tol)
        assert (m == rr.DEPTH).sum() >= 1
        h.reproject(r, 0.0, redo=True)
        _, _, m0 = check("two quads, tolerance 0", r, h, s, hist, prev, 0.0)
        assert not (m0 & rr.DEPTH).any() and np.array_equal(m == rr.DEPTH, (m0 == 0) & (m != 0))


# ---- the object over several frames and contexts ------------------------------------------------------------------------
def run_chain(frames, contexts):
    """The frames on one object, frame k on contexts[k % len]; [(warped, mask)] per frame, each checked."""
    from trident_raster import raster

    outs = []
    prev = None
    with raster.TriHistory(frames[0][0].width, frames[0][0].height) as h:
        for k, (s, hist) in enumerate(frames):
            r = contexts[k % len(contexts)]
            render(r, s, hist)
            h.reproject(r)
            prev, c, m = check(f"frame {k} on context {k % len(contexts)}", r, h, s, hist, prev)
            outs.append((c, m))
    return outs


def test_three_frames_on_one_and_on_two_contexts():
    """Two frames in flight are two contexts: the object gives what one context gives."""
    frames = chain()
    with open_raster(frames[0][0]) as a:
        one = run_chain(frames, [a])
        with open_raster(frames[0][0]) as b:
            two = run_chain(frames, [a, b])
    assert (one[0][1] == rr.NO_HISTORY).all() and (one[1][1] == 0).any() and (one[2][1] == 0).any()
    for k in range(3):
        assert np.array_equal(one[k][0], two[k][0]) and np.array_equal(one[k][1], two[k][1]), k


def test_redo_reads_the_same_previous_frame_again():
    from trident_raster import raster

    frames = chain()
    with open_raster(frames[0][0]) as r:
        fresh = run_chain(frames, [r])
        with raster.TriHistory(frames[0][0].width, frames[0][0].height) as h:
            render(r, *frames[0])
            h.reproject(r)
            f0 = snapshot(r)
            render(r, *frames[2])  # a frame that should not have been: it stores itself where frame 1 belongs
            h.reproject(r)
            render(r, *frames[1])
            h.reproject(r, redo=True)
            f1, c, m = check("redo", r, h, *frames[1], f0)
            assert np.array_equal(c, fresh[1][0]) and np.array_equal(m, fresh[1][1])
            render(r, *frames[2])
            h.reproject(r)
            _, c, m = check("after the redo", r, h, *frames[2], f1)
            assert np.array_equal(c, fresh[2][0]) and np.array_equal(m, fresh[2][1])
        with raster.TriHistory(frames[0][0].width, frames[0][0].height) as h:  # a redo first is a plain call
            render(r, *frames[0])
            h.reproject(r, redo=True)
            _, c, m = check("redo first", r, h, *frames[0], None)
            assert np.array_equal(m, fresh[0][1])


def test_the_pass_changes_nothing_of_the_context():
    from trident_raster import raster

    s = id_ref.cubes_and_quad()
    hist = mr.previous_frame(s)
    with open_raster(s) as r:
        render(r, s, hist)
        before = snapshot(r) + (r.read_motion(),)
        with raster.TriHistory(s.width, s.height) as h:
            for _ in range(2):
                render(r, s, hist)
                h.reproject(r)
                r.synchronize()
            after = snapshot(r) + (r.read_motion(),)
            h.read()
        render(r, s, hist)
        again = snapshot(r) + (r.read_motion(),)
    for a, b, c in zip(before, after, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8))


# ---- the C-ABI's rules ----------------------------------------------------------------------------------------------
def test_error_codes():
    import torch

    from trident_raster import abi, raster, scenes

    s = id_ref.cubes_and_quad()
    lib = raster.load_library()

    def code(call):
        with pytest.raises(raster.TriError) as ei:
            call()
        return ei.value.code

    def fails(call, rc, text):  # the code, and the whole of tri_last_error's text
        assert code(call) == rc
        assert lib.tri_last_error().decode() == text

    assert code(lambda: raster.TriHistory(0, 70)) == abi.TRI_E_INVALID
    assert code(lambda: raster.TriHistory(65536, 32769)) == abi.TRI_E_INVALID
    assert code(lambda: raster.TriHistory(16, 16, device=torch.cuda.device_count())) == abi.TRI_E_INVALID
    with raster.TriHistory(s.width, s.height) as h:
        assert code(h.read) == abi.TRI_E_STATE and code(h.images) == abi.TRI_E_STATE and code(h.timing) == abi.TRI_E_STATE
        fails(h.read, abi.TRI_E_STATE, "tri_history_read: no pass has run (tri_history_reproject)")
        fails(h.images, abi.TRI_E_STATE, "tri_history_get_output: no pass has run (tri_history_reproject)")
        fails(h.timing, abi.TRI_E_STATE, "tri_history_get_timing: no pass has run (tri_history_reproject)")
        off = "tri_history_reproject: the context's motion output is off (tri_set_motion_output)"
        with raster.TriRaster(s.width, s.height) as r:
            scenes.load_scene(r, s)
            fails(lambda: h.reproject(r), abi.TRI_E_STATE, off)  # the motion output is off
            r.set_id_output(True)
            r.render_frame()
            fails(lambda: h.reproject(r), abi.TRI_E_STATE, off)
            r.set_motion_output(True)
            fails(lambda: h.reproject(r), abi.TRI_E_STATE,  # on, but no frame yet
                  "tri_history_reproject: no frame was rendered with the motion output on")
            r.render_frame()
            params = abi.TriReprojectParams(0.0, 0)
            assert lib.tri_history_reproject(None, r._ctx, C.byref(params)) == abi.TRI_E_INVALID
            assert lib.tri_history_reproject(h._h, None, C.byref(params)) == abi.TRI_E_INVALID
            assert lib.tri_history_reproject(h._h, r._ctx, None) == abi.TRI_E_INVALID
            for tol in (-1.0, -1e-30, float("nan"), float("inf")):
                assert code(lambda: h.reproject(r, tol)) == abi.TRI_E_INVALID, tol
            for flags in (2, 3, 0x80000000):
                assert code(lambda: h.reproject(r, flags=flags)) == abi.TRI_E_INVALID, flags
            fails(h.read, abi.TRI_E_STATE, "tri_history_read: no pass has run (tri_history_reproject)")  # none of these ran a pass
            h.reproject(r)
            _, m = h.read()
            assert (m == rr.NO_HISTORY).all()
            assert lib.tri_history_read(h._h, None, None) == abi.TRI_OK
            r.set_motion_output(False)
            fails(lambda: h.reproject(r), abi.TRI_E_STATE, off)
        for w, hh in ((s.width + 1, s.height), (s.height, s.width)):  # another extent
            with open_raster(id_ref.cubes_and_quad(w, hh)) as other:
                other.render_frame()
                fails(lambda: h.reproject(other), abi.TRI_E_INVALID,
                      f"tri_history_reproject: the context is {w} x {hh}, the history {s.width} x {s.height}")
        with open_raster(s, band=(16, 48)) as band:  # a row band
            band.render_frame()
            fails(lambda: h.reproject(band), abi.TRI_E_UNSUPPORTED,
                  "tri_history_reproject: a row-band context (the fetch leaves the band)")
        if torch.cuda.device_count() > 1:  # another device
            with open_raster(s, device=1) as far:
                far.render_frame()
                fails(lambda: h.reproject(far), abi.TRI_E_INVALID,
                      "tri_history_reproject: the context is on device 1, the history on 0")


def test_images_and_timing():
    from trident_raster import abi, raster

    s = id_ref.sphere_and_quad()
    hist = mr.previous_frame(s)
    with open_raster(s) as r, raster.TriHistory(s.width, s.height) as h:
        render(r, s, hist)
        h.reproject(r)
        col, mask = h.images()
        assert (col.width, col.height, col.pitch_bytes, col.format) == (s.width, s.height, s.width * 4, abi.TRI_FORMAT_B8G8R8A8_UNORM)
        assert (mask.width, mask.height, mask.pitch_bytes, mask.format) == (s.width, s.height, s.width, abi.TRI_FORMAT_R8_UINT)
        assert col.device_ptr and mask.device_ptr and col.device == mask.device == r.output_image().device
        assert col.device_ptr % 16 == 0 and mask.device_ptr % 16 == 0
        assert h.timing() == (0.0, 0)  # the context asked for no timed frame
        r.set_timing(True)
        for k in range(3):
            r.render()
            h.reproject(r)
            r.synchronize()
            assert h.timing()[1] == k + 1
        ms, passes = h.timing()
        t = r.timing()
        print(f"REPROJECT timing: {1e3 * ms / passes:.1f} us per pass in k_reproject, stages {t}")
        assert passes == 3 and ms > 0.0 and t["frames"] == 3
        r.set_timing(False)
        r.render()
        h.reproject(r)
        assert h.timing() == (ms, 3)
