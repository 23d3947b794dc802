"""GPU tests of temporal upscaling (include/tri_raster.h "temporal upscaling"): k_upscale_resolve, tri_upscale and its
place behind the frame.

The bar throughout: the device's accumulated colour (uint16), resolved image and mask == tests/upscale_ref.py's
restatement, fed with the device's own colour, ids and depth of each frame, the library's table (tri_motion_matrices) and
the restatement's OWN previous output as history, compared as bytes — ZERO mismatches at every frame of a jittered chain.
The shapes are the smallest at which the kernel can go wrong: 50 x 35 -> 100 x 70 (2 x; two output tiles across, a partial
one; mixed waves), 43 x 32 -> 64 x 48 (a ratio that is no integer), 37 x 23 -> 101 x 69 (nearly 3 x, both ratios odd, output
rows that are not 8-B aligned), 1 x 1 -> 1 x 1 and 1 x 1 -> 3 x 3, 22 x 2 -> 65 x 5 (a tile column one pixel wide, a partial
tile row, windows that clamp on both sides), 3 x 100 -> 3 x 200 (one axis at 1 x), 32 x 32 -> 64 x 64 under 1024 draws of
2 x 2 px (every lane pair gathers another table row, ids up to the table's end), and 37 x 23 -> 74 x 46 under caller-bound
targets at a 4-B offset.
"""
import ctypes as C

import numpy as np
import pytest

import id_ref
import motion_ref as mr
import reproject_ref as rr
import taa_ref as tr
import upscale_ref as ur

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


def jittered_frame(n, period, scene, hist):
    """Frame n of a chain under the jitter contract, over the RENDER extent: (the jitter, the scene under it, its motion
    history — the previous view, models and UNJITTERED projection under the same jitter; None: no history)."""
    from trident_raster import raster

    jx, jy = raster.taa_jitter(n, period)
    cur = tr.jittered(scene, jx, jy)
    return (jx, jy), cur, (None if hist is None else tr.contract_history(scene, jx, jy, *hist))


def check(tag, r, t, scene, hist, prev, jitter=(0.0, 0.0), alpha=0.1, reject=True):
    """The object's outputs against the restatement over the device's own frame; returns ((accumulated, ids): the next
    call's `prev`, from the RESTATEMENT; resolved; mask; the frame)."""
    from trident_raster import raster

    cur = snapshot(r)
    got_c, got_a, got_m = t.read()
    table = raster.motion_matrices(scene.ubo, scene.draws, hist)
    want_a, want_c, want_m = ur.restate(table, cur[0], cur[1], cur[2], prev, t.width, t.height, jitter, alpha, reject)
    bad_m = int((got_m != want_m).sum())
    bad_c = int((got_c != want_c).any(axis=-1).sum())
    bad_a = int((got_a != want_a).any(axis=-1).sum())
    counts = {k: int(((want_m & 15) == v).sum()) for k, v in (("valid", 0), ("none", 1), ("no_proj", 2), ("outside", 4), ("id", 8))}
    counts["clamped"] = int(((want_m & ur.CLAMPED) != 0).sum())
    counts["no_sample"] = int(((want_m & ur.NO_SAMPLE) != 0).sum())
    print(f"UPSCALE {tag}: {scene.width} x {scene.height} -> {t.width} x {t.height}, {counts}, mismatches: mask {bad_m}, "
          f"resolved {bad_c}, rgba16 {bad_a}")
    assert got_m.shape == want_m.shape and got_c.shape == want_c.shape and got_a.shape == want_a.shape
    assert bad_m == 0, f"{tag}: {bad_m} mask mismatches"
    assert bad_a == 0, f"{tag}: {bad_a} rgba16 mismatches"
    assert bad_c == 0, f"{tag}: {bad_c} resolved mismatches"
    assert np.array_equal(t.read_ids(), cur[0]), f"{tag}: the stored ids are not the frame's"
    return (want_a, cur[0]), got_c, got_m, cur


def chain_of(scene, frames=8):
    """`frames` consecutive unjittered frames ending in `scene`: [(scene, (prev_view, prev_projection, prev_models))], the
    first without history. Odd steps move camera and draws, even steps the camera alone and slightly."""
    out = []
    s = scene
    for k in range(frames - 1, 0, -1):
        if k % 2:
            hist = mr.previous_frame(s)
        else:
            hist = mr.previous_frame(s, still=tuple(range(len(s.draws))), camera_move=mr.rigid((0.02, 0.01, 0.0), (0.3, -0.4, 0.0)))
        out.append((s, hist))
        s = rr.previous_scene(s, hist)
    out.append((s, None))
    return out[::-1]


def run_chain(tag, frames, contexts, out, alpha=0.1, reject=True):
    """The frames, jittered, on one object of output extent `out`, frame k on contexts[k % len]; [(resolved, mask)] per
    frame, each checked."""
    from trident_raster import raster

    s0 = frames[0][0]
    period = raster.upscale_jitter_period(s0.width, s0.height, *out)
    outs, prev = [], None
    with raster.TriUpscale(s0.width, s0.height, *out) as t:
        for k, (s, hist) in enumerate(frames):
            r = contexts[k % len(contexts)]
            j, cur, h = jittered_frame(k, period, s, hist)
            render(r, cur, h)
            t.resolve(r, j, alpha, reject)
            prev, c, m, _ = check(f"{tag} / frame {k}", r, t, cur, h, prev, j, alpha, reject)
            outs.append((c, m))
    return outs


def mesh_chain(tag, rw, rh, ow, oh, **kw):
    frames = chain_of(id_ref.cubes_and_quad(rw, rh))
    with open_raster(frames[0][0], **kw) as r:
        return run_chain(tag, frames, [r], (ow, oh))


# ---- k_upscale_resolve over an 8-frame jittered chain: a moved camera and three moved draws ------------------------------
@pytest.mark.parametrize("rw,rh,ow,oh", [(50, 35, 100, 70), (43, 32, 64, 48), (37, 23, 101, 69), (22, 2, 65, 5), (3, 100, 3, 200)])
def test_three_moved_draws(rw, rh, ow, oh):
    outs = mesh_chain(f"cubes_{rw}x{rh}", rw, rh, ow, oh)
    assert (outs[0][1] == ur.NO_HISTORY).all()
    masks = np.stack([m for _, m in outs[1:]])
    assert ((masks & 15) == 0).any()
    if (rw, rh) == (50, 35):
        assert (masks == ur.OUTSIDE).any() and (masks == ur.ID).any() and (masks & ur.CLAMPED).any()
    if (rw, rh) == (37, 23):
        assert (masks & ur.NO_SAMPLE).any()  # nearly 3 x: samples more than an output pixel away


@pytest.mark.parametrize("ow,oh", [(1, 1), (3, 3)])
def test_one_render_pixel(ow, oh):
    s = id_ref.pixel_quads("upscale_1x1", 1, 1, [(0, 0, 1, 1, 0.5)])
    still = (*mr.camera_of(s.ubo), None)
    with open_raster(s) as r:
        outs = run_chain(f"1x1 -> {ow}x{oh}", [(s, None)] + [(s, still)] * 7, [r], (ow, oh))
    assert (outs[0][1] == ur.NO_HISTORY).all() and all((m & 15 == 0).all() for _, m in outs[1:])


def test_caller_bound_targets_at_a_4_byte_offset():
    """37 x 23 rendered into a caller's colour and depth that start 4 B past a 16-B boundary, resolved at 74 x 46."""
    import torch

    s = id_ref.cubes_and_quad(37, 23)
    frames = chain_of(s)
    n = s.width * s.height
    col = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
    dep = torch.zeros(n + 1, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert col[1:].data_ptr() % 16 == 4 and dep[1:].data_ptr() % 16 == 4
    with open_raster(s) as r:
        r.bind_output(col[1:].data_ptr(), dep[1:].data_ptr())
        outs = run_chain("bound", frames, [r], (74, 46))
        assert any(((m & 15) == 0).any() for _, m in outs[1:]) and any(((m & 15) != 0).any() for _, m in outs[1:])
        cur = snapshot(r)
        assert np.array_equal(col[1:].cpu().numpy().view(np.uint8).reshape(s.height, s.width, 4), cur[2])  # (it was the caller's)
        r.bind_output(None, None)


def test_1024_small_draws():
    """32 x 32 covered by 1024 quads of 1 x 1 render px — 2 x 2 px of the 64 x 64 output — each its own draw with its own
    whole-pixel translation one frame ago: every pair of lanes gathers another row, the last id is the table's last row."""
    w = h = 32
    rects = [(i, j, i + 1, j + 1, 0.25 + 0.5 * ((i * 7 + j * 3) % 16) / 16.0) for j in range(32) for i in range(32)]
    s = id_ref.pixel_quads("upscale_1024_quads", w, h, rects)
    v, p = mr.camera_of(s.ubo)
    shifts = [((k * 5) % 7 - 3, (k * 11) % 5 - 2) for k in range(1024)]
    prev = np.array([mr.to_cm(mr.rigid((tx, ty, 0.0))).reshape(16) for tx, ty in shifts], F)
    with open_raster(s) as r:
        outs = run_chain("1024 quads", [(s, None)] + [(s, (v, p, prev))] * 7, [r], (64, 64))
        assert r.read_ids().max() == 1024
    masks = np.stack([m for _, m in outs[1:]])
    assert ((masks & 15) == 0).any() and (masks == ur.ID).any() and (masks == ur.OUTSIDE).any()


# ---- the rule's cases ---------------------------------------------------------------------------------------------------
OUT2 = lambda s: (2 * s.width, 2 * s.height)  # noqa: E731


def test_first_pass_and_after_a_reset():
    from trident_raster import raster

    s = id_ref.cubes_and_quad(50, 35)
    still = (*mr.camera_of(s.ubo), None)
    with open_raster(s) as r, raster.TriUpscale(s.width, s.height, *OUT2(s)) as t:
        render(r, s, still)
        for tag in ("first", "after the reset"):
            t.resolve(r)
            prev, c, m, cur = check(tag, r, t, s, still, None)
            _, a, _ = t.read()
            near = ur.nearest(cur[2], t.width, t.height)
            assert (m == ur.NO_HISTORY).all() and np.array_equal(c, near)
            assert np.array_equal(a, near.astype(np.uint16) * 257)
            t.resolve(r)
            _, c, m, _ = check(tag + ", then", r, t, s, still, prev)
            # a still scene: every pixel valid; no jitter: k = 1 / 4 everywhere, and the history is the sample itself
            assert (m == 0).all() and np.array_equal(c, near)
            t.reset()


def test_a_previous_camera_turned_round():
    """Every point lay behind the previous camera: mask 2 everywhere, the history restarts."""
    from trident_raster import raster

    s = id_ref.cubes_and_quad(50, 35)
    hist = mr.previous_frame(s, camera_move=mr.rigid((0, 0, 0), (0.0, 180.0, 0.0)))
    with open_raster(s) as r, raster.TriUpscale(s.width, s.height, *OUT2(s)) as t:
        render(r, rr.previous_scene(s, hist), None)
        t.resolve(r)
        prev = check("turned / first", r, t, rr.previous_scene(s, hist), None, None)[0]
        render(r, s, hist)
        t.resolve(r)
        _, c, m, cur = check("turned", r, t, s, hist, prev)
        assert (m == ur.NO_PROJ).all() and np.array_equal(c, ur.nearest(cur[2], t.width, t.height))


@pytest.mark.parametrize("reject", [True, False])
def test_a_quad_moved_aside(reject):
    """The quad stood 10 render px to the right. With the id test: ID exactly where no 3 x 3 previous render neighbour
    shows the pixel's id. Without: no ID at all, and the clamp deals with the stale colour."""
    from trident_raster import raster

    w, h = 32, 24
    s = id_ref.pixel_quads("upscale_moved_quad", w, h, [(5, 4, 17, 20, 0.5)])
    v, p = mr.camera_of(s.ubo)
    hist = (v, p, np.array([mr.to_cm(mr.rigid((10.0, 0.0, 0.0))).reshape(16)], F))
    was = rr.previous_scene(s, hist)
    with open_raster(s) as r, raster.TriUpscale(w, h, 64, 48) as t:
        render(r, was, None)
        t.resolve(r, reject_ids=reject)
        prev, _, _, before = check("moved / first", r, t, was, None, None, reject=reject)
        render(r, s, hist)
        t.resolve(r, reject_ids=reject)
        _, c, m, cur = check(f"moved, reject {reject}", r, t, s, hist, prev, reject=reject)
    up = lambda a: ur.nearest(a, 64, 48)  # noqa: E731
    if reject:
        # the background did not move: its previous place is its own, and the window there is the render pixel's
        near_same = tr.window(before[0] == 0, np.logical_or)
        assert np.array_equal(m == ur.ID, up((cur[0] == 0) & ~near_same)) and (m == ur.ID).sum() > 0
        assert (m[up(cur[0] == 1)] & 15 == 0).all()
    else:
        assert not (m & ur.ID).any() and (m & ur.CLAMPED).any()
        far = up((cur[0] == 0) & ~tr.window(cur[0] == 1, np.logical_or))
        assert np.array_equal(c[far], up(cur[2])[far])  # one colour in the window: clamped to the current frame


def test_alpha_one():
    """alpha = 1: parity over a chain, and where the sample lies on the output pixel's centre (k = 1) a valid pixel is the
    current sample exactly. A jitter of (0.25, 0.25) at 2 x puts render pixel (x, y)'s sample on the centre of output
    pixel (2 x, 2 y): k = 1 on a quarter of the pixels."""
    from trident_raster import raster

    frames = chain_of(id_ref.cubes_and_quad(50, 35), 3)
    s, hist = frames[-1]
    j = (F(0.25), F(0.25))
    with open_raster(frames[0][0]) as r:
        outs = run_chain("alpha 1", frames, [r], (100, 70), alpha=1.0)
        assert (outs[-1][1] & 15 == 0).any()
        cur, h = tr.jittered(s, *j), tr.contract_history(s, *j, *hist)
        with raster.TriUpscale(50, 35, 100, 70) as t:
            prev = None
            for n in range(2):
                render(r, cur, h)
                t.resolve(r, j, 1.0)
                prev, c, m, frame = check(f"alpha 1, k = 1 / pass {n}", r, t, cur, h, prev, j, 1.0)
    xr, yr, k = ur.sample(50, 35, 100, 70, *j)
    on_centre = (k == F(1.0)) & ((m & 15) == 0)
    assert (k == F(1.0)).sum() == 50 * 35 and on_centre.sum() > 0.5 * 50 * 35
    assert np.array_equal(c[on_centre], frame[2][yr, xr][on_centre])
    assert not (m[k == F(1.0)] & ur.NO_SAMPLE).any()


def test_three_frames_on_one_and_on_two_contexts():
    """Two frames in flight are two contexts: the object gives what one context gives."""
    frames = chain_of(id_ref.cubes_and_quad(50, 35), 3)
    with open_raster(frames[0][0]) as a:
        one = run_chain("one context", frames, [a], (100, 70))
        with open_raster(frames[0][0]) as b:
            two = run_chain("two contexts", frames, [a, b], (100, 70))
    assert (one[0][1] == ur.NO_HISTORY).all() and (one[1][1] & 15 == 0).any() and (one[2][1] & 15 == 0).any()
    for k in range(3):
        assert np.array_equal(one[k][0], two[k][0]) and np.array_equal(one[k][1], two[k][1]), k


def test_redo_reads_the_same_history_again():
    from trident_raster import raster

    frames = chain_of(id_ref.cubes_and_quad(50, 35), 3)
    s0 = frames[0][0]
    out = (100, 70)
    period = raster.upscale_jitter_period(s0.width, s0.height, *out)
    jf = [jittered_frame(k, period, s, hist) for k, (s, hist) in enumerate(frames)]
    with open_raster(s0) as r:
        fresh = run_chain("fresh", frames, [r], out)
        with raster.TriUpscale(s0.width, s0.height, *out) as t:
            render(r, *jf[0][1:])
            t.resolve(r, jf[0][0])
            p0 = check("redo / frame 0", r, t, *jf[0][1:], None, jf[0][0])[0]
            render(r, *jf[2][1:])  # a frame that should not have been: it stores itself where frame 1 belongs
            t.resolve(r, jf[2][0])
            render(r, *jf[1][1:])
            t.resolve(r, jf[1][0], redo=True)
            p1, c, m, _ = check("redo", r, t, *jf[1][1:], p0, jf[1][0])
            assert np.array_equal(c, fresh[1][0]) and np.array_equal(m, fresh[1][1])
            render(r, *jf[2][1:])
            t.resolve(r, jf[2][0])
            _, c, m, _ = check("after the redo", r, t, *jf[2][1:], p1, jf[2][0])
            assert np.array_equal(c, fresh[2][0]) and np.array_equal(m, fresh[2][1])
        with raster.TriUpscale(s0.width, s0.height, *out) as t:  # a redo first is a plain call
            render(r, *jf[0][1:])
            t.resolve(r, jf[0][0], redo=True)
            _, c, m, _ = check("redo first", r, t, *jf[0][1:], None, jf[0][0])
            assert np.array_equal(m, fresh[0][1])


def test_the_pass_changes_nothing_of_the_context():
    from trident_raster import raster

    s = id_ref.cubes_and_quad(50, 35)
    hist = mr.previous_frame(s)
    with open_raster(s) as r:
        render(r, s, hist)
        before = snapshot(r) + (r.read_motion(),)
        with raster.TriUpscale(s.width, s.height, *OUT2(s)) as t:
            for _ in range(2):
                render(r, s, hist)
                t.resolve(r)
                r.synchronize()
            after = snapshot(r) + (r.read_motion(),)
            t.read()
        render(r, s, hist)
        again = snapshot(r) + (r.read_motion(),)
    for a, b, c in zip(before, after, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8))


# ---- the C-ABI's rules ------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch

    from trident_raster import abi, raster, scenes

    s = id_ref.cubes_and_quad(50, 35)
    lib = raster.load_library()

    def code(call):
        with pytest.raises(raster.TriError) as ei:
            call()
        return ei.value.code

    def fails(call, rc, text):  # the code, and the whole of tri_last_error's text
        assert code(call) == rc
        assert lib.tri_last_error().decode() == text

    for bad in [(0, 35, 100, 70), (50, 35, 49, 70), (50, 35, 100, 34), (50, 35, 151, 70), (50, 35, 100, 106),
                (65536, 32768, 65536, 32769)]:
        assert code(lambda: raster.TriUpscale(*bad)) == abi.TRI_E_INVALID, bad
    assert code(lambda: raster.TriUpscale(16, 16, 32, 32, device=torch.cuda.device_count())) == abi.TRI_E_INVALID
    with raster.TriUpscale(s.width, s.height, *OUT2(s)) as t:
        assert code(t.read) == abi.TRI_E_STATE and code(t.images) == abi.TRI_E_STATE and code(t.timing) == abi.TRI_E_STATE
        fails(t.read, abi.TRI_E_STATE, "tri_upscale_read: no pass has run (tri_upscale_resolve)")
        fails(t.images, abi.TRI_E_STATE, "tri_upscale_get_output: no pass has run (tri_upscale_resolve)")
        fails(t.timing, abi.TRI_E_STATE, "tri_upscale_get_timing: no pass has run (tri_upscale_resolve)")
        off = "tri_upscale_resolve: the context's motion output is off (tri_set_motion_output)"
        fails(t.read_ids, abi.TRI_E_STATE, "tri_upscale_read_ids: no pass has run (tri_upscale_resolve)")
        with raster.TriRaster(s.width, s.height) as r:
            scenes.load_scene(r, s)
            fails(lambda: t.resolve(r), abi.TRI_E_STATE, off)  # the motion output is off
            r.set_id_output(True)
            r.render_frame()
            fails(lambda: t.resolve(r), abi.TRI_E_STATE, off)
            r.set_motion_output(True)
            fails(lambda: t.resolve(r), abi.TRI_E_STATE,  # on, but no frame yet
                  "tri_upscale_resolve: no frame was rendered with the motion output on")
            r.render_frame()
            fails(lambda: t.blit(r, s.width, s.height), abi.TRI_E_STATE,  # no pass has run
                  "tri_upscale_blit_linear: no pass has run (tri_upscale_resolve)")
            params = abi.TriUpscaleParams(0.1, (C.c_float * 2)(0.0, 0.0), 0)
            assert lib.tri_upscale_resolve(None, r._ctx, C.byref(params)) == abi.TRI_E_INVALID
            assert lib.tri_upscale_resolve(t._h, None, C.byref(params)) == abi.TRI_E_INVALID
            assert lib.tri_upscale_resolve(t._h, r._ctx, None) == abi.TRI_E_INVALID
            for alpha in (0.0, -0.1, 1.0000001, 2.0, float("nan"), float("inf"), float("-inf")):
                assert code(lambda: t.resolve(r, alpha=alpha)) == abi.TRI_E_INVALID, alpha
            for j in (0.5000001, -0.5000001, 1.0, float("nan"), float("inf"), float("-inf")):
                assert code(lambda: t.resolve(r, (j, 0.0))) == abi.TRI_E_INVALID, j
                assert code(lambda: t.resolve(r, (0.0, j))) == abi.TRI_E_INVALID, j
            for flags in (4, 7, 0x80000000):
                assert code(lambda: t.resolve(r, flags=flags)) == abi.TRI_E_INVALID, flags
            fails(t.read, abi.TRI_E_STATE, "tri_upscale_read: no pass has run (tri_upscale_resolve)")  # none of these ran a pass
            t.resolve(r, (-0.5, 0.5))
            _, _, m = t.read()
            assert (m == ur.NO_HISTORY).all()
            assert lib.tri_upscale_read(t._h, None, None, None) == abi.TRI_OK
            assert lib.tri_upscale_read_ids(t._h, None) == abi.TRI_OK
            assert lib.tri_upscale_get_output(t._h, None, None, None) == abi.TRI_OK
            assert code(lambda: t.blit(r, 0, 4)) == abi.TRI_E_INVALID
            r.set_motion_output(False)
            fails(lambda: t.resolve(r), abi.TRI_E_STATE, off)
        # a context of another extent — the object's OUTPUT extent included
        for w, hh in ((s.width + 1, s.height), (s.height, s.width), OUT2(s)):
            with open_raster(id_ref.cubes_and_quad(w, hh)) as other:
                other.render_frame()
                extent = f"the context is {w} x {hh}, the history {s.width} x {s.height} (the render extent)"
                fails(lambda: t.resolve(other), abi.TRI_E_INVALID, "tri_upscale_resolve: " + extent)
                fails(lambda: t.blit(other, 8, 8), abi.TRI_E_INVALID, "tri_upscale_blit_linear: " + extent)
        with open_raster(s, band=(16, 32)) as band:  # a row band
            band.render_frame()
            fails(lambda: t.resolve(band), abi.TRI_E_UNSUPPORTED, "tri_upscale_resolve: a row-band context (the samples and the 3 x 3 windows leave the band)")
            fails(lambda: t.blit(band, 8, 8), abi.TRI_E_STATE, "tri_upscale_blit_linear: a row-band context has no whole frame")
        if torch.cuda.device_count() > 1:  # another device
            with open_raster(s, device=1) as far:
                far.render_frame()
                fails(lambda: t.resolve(far), abi.TRI_E_INVALID,
                      "tri_upscale_resolve: the context is on device 1, the history on 0 (the render extent)")


def test_images_blit_and_timing():
    import torch

    from trident_raster import abi, raster

    s = id_ref.sphere_and_quad(50, 35)
    ow, oh = 100, 70
    frames = chain_of(s, 2)
    period = raster.upscale_jitter_period(s.width, s.height, ow, oh)
    with open_raster(s) as r, raster.TriUpscale(s.width, s.height, ow, oh) as t:
        seen = []
        for k, (sc_, hist) in enumerate(frames):
            j, cur, h = jittered_frame(k, period, sc_, hist)
            render(r, cur, h)
            t.resolve(r, j)
            col, acc, mask = t.images()
            assert (col.width, col.height, col.pitch_bytes, col.format) == (ow, oh, ow * 4, abi.TRI_FORMAT_B8G8R8A8_UNORM)
            assert (acc.width, acc.height, acc.pitch_bytes, acc.format) == (ow, oh, ow * 8, abi.TRI_FORMAT_R16G16B16A16_UNORM)
            assert (mask.width, mask.height, mask.pitch_bytes, mask.format) == (ow, oh, ow, abi.TRI_FORMAT_R8_UINT)
            assert col.device_ptr and acc.device_ptr and mask.device_ptr and col.device == acc.device == mask.device == r.output_image().device
            assert col.device_ptr % 16 == 0 and acc.device_ptr % 16 == 0
            seen.append(acc.device_ptr)
            # colour16 is the set the last pass wrote: its bytes are tri_upscale_read's rgba16
            res, a16, m8 = t.read()
            raw = raster.copy_device_to_host(acc.device_ptr, oh * acc.pitch_bytes, acc.device)
            assert np.array_equal(raw.view(np.uint16).reshape(oh, ow, 4), a16)
            raw = raster.copy_device_to_host(col.device_ptr, oh * col.pitch_bytes, col.device)
            assert np.array_equal(raw.reshape(oh, ow, 4), res)
            raw = raster.copy_device_to_host(mask.device_ptr, oh * mask.pitch_bytes, mask.device)
            assert np.array_equal(raw.reshape(oh, ow), m8)
        assert seen[0] != seen[1]  # the two sets alternate
        # the presentation blit at the output extent is the resolved image
        t.blit(r, ow, oh)
        assert np.array_equal(r.read_present(), res)
        r.blit(s.width, s.height)
        assert np.array_equal(r.read_present(), snapshot(r)[2])  # ... and tri_blit_linear still shows the raw frame
        out = torch.zeros(ow * oh, dtype=torch.int32, device="cuda:0")
        t.blit(r, ow, oh, out.data_ptr())
        r.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint8).reshape(oh, ow, 4), res)
        t.blit(r, 2 * ow, oh // 2)
        assert r.read_present().shape == (oh // 2, 2 * ow, 4)

        assert t.timing() == (0.0, 0)  # the context asked for no timed frame
        r.set_timing(True)
        for k in range(3):
            r.render()
            t.resolve(r)
            r.synchronize()
            assert t.timing()[1] == k + 1
        ms, passes = t.timing()
        tm = r.timing()
        print(f"UPSCALE timing: {1e3 * ms / passes:.1f} us per pass in k_upscale_resolve and the id copy, stages {tm}")
        assert passes == 3 and ms > 0.0 and tm["frames"] == 3
        r.set_timing(False)
        r.render()
        t.resolve(r)
        assert t.timing() == (ms, 3)
