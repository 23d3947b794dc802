"""GPU tests of temporal anti-aliasing (include/tri_raster.h "temporal anti-aliasing"): k_taa_resolve, tri_taa and its
place behind the frame.

The bar throughout: the device's accumulated colour (uint16), resolved image and mask == tests/taa_ref.py's restatement,
fed with the device's own colour, ids and depth of each frame, the library's table (tri_motion_matrices) and the
restatement's OWN previous output as history, compared as bytes — ZERO mismatches at every frame of a jittered chain:
the rule fixes every operation, and an error in one frame's history would otherwise hide in the next. The shapes are the
smallest at which the kernel can go wrong: 100 x 70 (two tiles across, a partial one; mixed waves), 101 x 70 (rows that
are not 8-B aligned), 37 x 23 under caller-bound targets at a 4-B offset, 65 x 5 and 3 x 200 (a tile's second column one
pixel wide, a partial tile row; windows that clamp on both sides at once), 1 x 1, and 64 x 64 under 1024 draws of 2 x 2 px
(every lane gathers another table row, ids up to the table's end).
"""
import ctypes as C

import numpy as np
import pytest

import id_ref
import motion_ref as mr
import reproject_ref as rr
import taa_ref as tr

pytestmark = pytest.mark.gpu
F = np.float32
PERIOD = 8


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


def jittered_frame(n, scene, hist):
    """Frame n of a chain under the jitter contract: (the scene under jitter n, its motion history — the previous view,
    models and UNJITTERED projection under the same jitter; None: no history)."""
    from trident_raster import raster

    jx, jy = raster.taa_jitter(n, PERIOD)
    cur = tr.jittered(scene, jx, jy)
    return cur, (None if hist is None else tr.contract_history(scene, jx, jy, *hist))


def check(tag, r, t, scene, hist, prev, alpha=0.1, reject=True):
    """The object's outputs against the restatement over the device's own frame; returns ((accumulated, ids): the next
    call's `prev`, from the RESTATEMENT; resolved; mask; the frame)."""
    from trident_raster import raster

    cur = snapshot(r)
    got_c, got_a, got_m = t.read()
    table = raster.motion_matrices(scene.ubo, scene.draws, hist)
    want_a, want_c, want_m = tr.restate(table, cur[0], cur[1], cur[2], prev, scene.width, scene.height, alpha, reject)
    bad_m = int((got_m != want_m).sum())
    bad_c = int((got_c != want_c).any(axis=-1).sum())
    bad_a = int((got_a != want_a).any(axis=-1).sum())
    counts = {k: int(((want_m & 15) == v).sum()) for k, v in (("valid", 0), ("none", 1), ("no_proj", 2), ("outside", 4), ("id", 8))}
    counts["clamped"] = int(((want_m & tr.CLAMPED) != 0).sum())
    print(f"TAA {tag}: {scene.width} x {scene.height}, {counts}, mismatches: mask {bad_m}, resolved {bad_c}, rgba16 {bad_a}")
    assert got_m.shape == want_m.shape and got_c.shape == want_c.shape and got_a.shape == want_a.shape
    assert bad_m == 0, f"{tag}: {bad_m} mask mismatches"
    assert bad_a == 0, f"{tag}: {bad_a} rgba16 mismatches"
    assert bad_c == 0, f"{tag}: {bad_c} resolved mismatches"
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


def run_chain(tag, frames, contexts, alpha=0.1, reject=True, taa=None):
    """The frames, jittered, on one object, frame k on contexts[k % len]; [(resolved, mask)] per frame, each checked."""
    from trident_raster import raster

    outs, prev = [], None
    t = taa or raster.TriTaa(frames[0][0].width, frames[0][0].height)
    try:
        for k, (s, hist) in enumerate(frames):
            r = contexts[k % len(contexts)]
            cur, h = jittered_frame(k, s, hist)
            render(r, cur, h)
            t.resolve(r, alpha, reject)
            prev, c, m, _ = check(f"{tag} / frame {k}", r, t, cur, h, prev, alpha, reject)
            outs.append((c, m))
    finally:
        if taa is None:
            t.close()
    return outs


def mesh_chain(tag, w, h, **kw):
    frames = chain_of(id_ref.cubes_and_quad(w, h))
    with open_raster(frames[0][0], **kw) as r:
        return run_chain(tag, frames, [r])


# ---- k_taa_resolve over an 8-frame jittered chain ---------------------------------------------------------------------------
def test_three_moved_draws():
    outs = mesh_chain("cubes", 100, 70)
    assert (outs[0][1] == tr.NO_HISTORY).all()
    masks = np.stack([m for _, m in outs[1:]])
    assert ((masks & 15) == 0).any() and (masks == tr.OUTSIDE).any() and (masks == tr.ID).any() and (masks & tr.CLAMPED).any()


def test_a_width_of_101():
    """Rows of 404 B (the history's of 808 B): the second tile column is 37 pixels wide, rows start at every 4-B phase."""
    outs = mesh_chain("cubes_101", 101, 70)
    assert any(((m & 15) == 0).any() for _, m in outs[1:])


@pytest.mark.parametrize("w,h", [(65, 5), (3, 200)])
def test_tile_and_halo_edges(w, h):
    """65 x 5: a tile column one pixel wide and a second tile row one pixel high; 3 x 200: 50 tiles of 3 lanes a row,
    every pixel's windows on a border."""
    outs = mesh_chain(f"cubes_{w}x{h}", w, h)
    assert any(((m & 15) == 0).any() for _, m in outs[1:])


def test_one_pixel():
    s = id_ref.pixel_quads("taa_1x1", 1, 1, [(0, 0, 1, 1, 0.5)])
    still = (*mr.camera_of(s.ubo), None)
    with open_raster(s) as r:
        outs = run_chain("1x1", [(s, None)] + [(s, still)] * 7, [r])
    assert outs[0][1][0, 0] == tr.NO_HISTORY and all((m & 15 == 0).all() for _, m in outs[1:])


def test_caller_bound_targets_at_a_4_byte_offset():
    """37 x 23 rendered into a caller's colour and depth that start 4 B past a 16-B boundary."""
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
        outs = run_chain("bound", frames, [r])
        assert any(((m & 15) == 0).any() for _, m in outs[1:]) and any(((m & 15) != 0).any() for _, m in outs[1:])
        cur = snapshot(r)
        assert np.array_equal(col[1:].cpu().numpy().view(np.uint8).reshape(s.height, s.width, 4), cur[2])  # (it was the caller's)
        r.bind_output(None, None)


def test_1024_small_draws():
    """64 x 64 covered by 1024 quads of 2 x 2 px, each its own draw with its own whole-pixel translation one frame ago:
    every lane gathers another row, the last id is the table's last row."""
    w = h = 64
    rects = [(2 * i, 2 * j, 2 * i + 2, 2 * j + 2, 0.25 + 0.5 * ((i * 7 + j * 3) % 16) / 16.0) for j in range(32) for i in range(32)]
    s = id_ref.pixel_quads("taa_1024_quads", w, h, rects)
    v, p = mr.camera_of(s.ubo)
    shifts = [((k * 5) % 13 - 6, (k * 11) % 9 - 4) for k in range(1024)]
    prev = np.array([mr.to_cm(mr.rigid((tx, ty, 0.0))).reshape(16) for tx, ty in shifts], F)
    with open_raster(s) as r:
        outs = run_chain("1024 quads", [(s, None)] + [(s, (v, p, prev))] * 7, [r])
        assert r.read_ids().max() == 1024
    masks = np.stack([m for _, m in outs[1:]])
    assert ((masks & 15) == 0).any() and (masks == tr.ID).any() and (masks == tr.OUTSIDE).any()


# ---- the rule's cases -----------------------------------------------------------------------------------------------------
def test_first_pass_and_after_a_reset():
    from trident_raster import raster

    s = id_ref.cubes_and_quad()
    still = (*mr.camera_of(s.ubo), None)
    with open_raster(s) as r, raster.TriTaa(s.width, s.height) as t:
        render(r, s, still)
        for tag in ("first", "after the reset"):
            t.resolve(r)
            prev, c, m, cur = check(tag, r, t, s, still, None)
            _, a, _ = t.read()
            assert (m == tr.NO_HISTORY).all() and np.array_equal(c, cur[2])
            assert np.array_equal(a, cur[2].astype(np.uint16) * 257)
            t.resolve(r)
            _, c, m, _ = check(tag + ", then", r, t, s, still, prev)
            assert (m == 0).all() and np.array_equal(c, cur[2])  # a still, unjittered scene: nothing moves
            t.reset()


def test_a_previous_camera_turned_round():
    """Every point lay behind the previous camera: mask 2 everywhere, the history restarts."""
    from trident_raster import raster

    s = id_ref.cubes_and_quad()
    hist = mr.previous_frame(s, camera_move=mr.rigid((0, 0, 0), (0.0, 180.0, 0.0)))
    with open_raster(s) as r, raster.TriTaa(s.width, s.height) as t:
        render(r, rr.previous_scene(s, hist), None)
        t.resolve(r)
        prev = check("turned / first", r, t, rr.previous_scene(s, hist), None, None)[0]
        render(r, s, hist)
        t.resolve(r)
        _, c, m, cur = check("turned", r, t, s, hist, prev)
        assert (m == tr.NO_PROJ).all() and np.array_equal(c, cur[2])


@pytest.mark.parametrize("reject", [True, False])
def test_a_quad_moved_aside(reject):
    """The quad stood 20 px to the right. With the id test: ID exactly where no 3 x 3 previous neighbour shows the
    pixel's id — the uncovered background less the column next to where the quad still is. Without: no ID at all, and
    the clamp deals with the stale colour."""
    from trident_raster import raster

    w, h = 64, 48
    s = id_ref.pixel_quads("taa_moved_quad", w, h, [(10, 8, 34, 40, 0.5)])
    v, p = mr.camera_of(s.ubo)
    hist = (v, p, np.array([mr.to_cm(mr.rigid((20.0, 0.0, 0.0))).reshape(16)], F))
    was = rr.previous_scene(s, hist)
    with open_raster(s) as r, raster.TriTaa(w, h) as t:
        render(r, was, None)
        t.resolve(r, reject_ids=reject)
        prev, _, _, before = check("moved / first", r, t, was, None, None, reject=reject)
        render(r, s, hist)
        t.resolve(r, reject_ids=reject)
        _, c, m, cur = check(f"moved, reject {reject}", r, t, s, hist, prev, reject=reject)
    # the background did not move: its previous place is its own, and some 3 x 3 previous neighbour there was background
    near_same = tr.window(before[0] == 0, np.logical_or)
    if reject:
        bg_was_quad = (cur[0] == 0) & (before[0] == 1)
        assert np.array_equal(m == tr.ID, (cur[0] == 0) & ~near_same) and (m == tr.ID).sum() > 0.8 * bg_was_quad.sum()
        assert (m[cur[0] == 1] & 15 == 0).all()
    else:
        assert not (m & tr.ID).any() and (m & tr.CLAMPED).any()
        far = (cur[0] == 0) & ~tr.window(cur[0] == 1, np.logical_or)
        assert np.array_equal(c[far], cur[2][far])  # one colour in the window: clamped to the current frame


def test_alpha_one_gives_the_current_frame():
    frames = chain_of(id_ref.cubes_and_quad(), 3)
    with open_raster(frames[0][0]) as r:
        outs = run_chain("alpha 1", frames, [r], alpha=1.0)
        assert np.array_equal(outs[-1][0], snapshot(r)[2])


def test_three_frames_on_one_and_on_two_contexts():
    """Two frames in flight are two contexts: the object gives what one context gives."""
    frames = chain_of(id_ref.cubes_and_quad(), 3)
    with open_raster(frames[0][0]) as a:
        one = run_chain("one context", frames, [a])
        with open_raster(frames[0][0]) as b:
            two = run_chain("two contexts", frames, [a, b])
    assert (one[0][1] == tr.NO_HISTORY).all() and (one[1][1] & 15 == 0).any() and (one[2][1] & 15 == 0).any()
    for k in range(3):
        assert np.array_equal(one[k][0], two[k][0]) and np.array_equal(one[k][1], two[k][1]), k


def test_redo_reads_the_same_history_again():
    from trident_raster import raster

    frames = chain_of(id_ref.cubes_and_quad(), 3)
    jf = [jittered_frame(k, s, hist) for k, (s, hist) in enumerate(frames)]
    with open_raster(frames[0][0]) as r:
        fresh = run_chain("fresh", frames, [r])
        with raster.TriTaa(frames[0][0].width, frames[0][0].height) as t:
            render(r, *jf[0])
            t.resolve(r)
            p0 = check("redo / frame 0", r, t, *jf[0], None)[0]
            render(r, *jf[2])  # a frame that should not have been: it stores itself where frame 1 belongs
            t.resolve(r)
            render(r, *jf[1])
            t.resolve(r, redo=True)
            p1, c, m, _ = check("redo", r, t, *jf[1], p0)
            assert np.array_equal(c, fresh[1][0]) and np.array_equal(m, fresh[1][1])
            render(r, *jf[2])
            t.resolve(r)
            _, c, m, _ = check("after the redo", r, t, *jf[2], p1)
            assert np.array_equal(c, fresh[2][0]) and np.array_equal(m, fresh[2][1])
        with raster.TriTaa(frames[0][0].width, frames[0][0].height) as t:  # a redo first is a plain call
            render(r, *jf[0])
            t.resolve(r, redo=True)
            _, c, m, _ = check("redo first", r, t, *jf[0], None)
            assert np.array_equal(m, fresh[0][1])


def test_the_pass_changes_nothing_of_the_context():
    from trident_raster import raster

    s = id_ref.cubes_and_quad()
    hist = mr.previous_frame(s)
    with open_raster(s) as r:
        render(r, s, hist)
        before = snapshot(r) + (r.read_motion(),)
        with raster.TriTaa(s.width, s.height) as t:
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

    assert code(lambda: raster.TriTaa(0, 70)) == abi.TRI_E_INVALID
    assert code(lambda: raster.TriTaa(65536, 32769)) == abi.TRI_E_INVALID
    assert code(lambda: raster.TriTaa(16, 16, device=torch.cuda.device_count())) == abi.TRI_E_INVALID
    with raster.TriTaa(s.width, s.height) as t:
        assert code(t.read) == abi.TRI_E_STATE and code(t.images) == abi.TRI_E_STATE and code(t.timing) == abi.TRI_E_STATE
        fails(t.read, abi.TRI_E_STATE, "tri_taa_read: no pass has run (tri_taa_resolve)")
        fails(t.images, abi.TRI_E_STATE, "tri_taa_get_output: no pass has run (tri_taa_resolve)")
        fails(t.timing, abi.TRI_E_STATE, "tri_taa_get_timing: no pass has run (tri_taa_resolve)")
        off = "tri_taa_resolve: the context's motion output is off (tri_set_motion_output)"
        with raster.TriRaster(s.width, s.height) as r:
            scenes.load_scene(r, s)
            fails(lambda: t.resolve(r), abi.TRI_E_STATE, off)  # the motion output is off
            r.set_id_output(True)
            r.render_frame()
            fails(lambda: t.resolve(r), abi.TRI_E_STATE, off)
            r.set_motion_output(True)
            fails(lambda: t.resolve(r), abi.TRI_E_STATE,  # on, but no frame yet
                  "tri_taa_resolve: no frame was rendered with the motion output on")
            r.render_frame()
            fails(lambda: t.blit(r, s.width, s.height), abi.TRI_E_STATE,  # no pass has run
                  "tri_taa_blit_linear: no pass has run (tri_taa_resolve)")
            params = abi.TriTaaParams(0.1, 0)
            assert lib.tri_taa_resolve(None, r._ctx, C.byref(params)) == abi.TRI_E_INVALID
            assert lib.tri_taa_resolve(t._h, None, C.byref(params)) == abi.TRI_E_INVALID
            assert lib.tri_taa_resolve(t._h, r._ctx, None) == abi.TRI_E_INVALID
            for alpha in (0.0, -0.1, 1.0000001, 2.0, float("nan"), float("inf"), float("-inf")):
                assert code(lambda: t.resolve(r, alpha)) == abi.TRI_E_INVALID, alpha
            for flags in (4, 7, 0x80000000):
                assert code(lambda: t.resolve(r, flags=flags)) == abi.TRI_E_INVALID, flags
            fails(t.read, abi.TRI_E_STATE, "tri_taa_read: no pass has run (tri_taa_resolve)")  # none of these ran a pass
            t.resolve(r)
            _, _, m = t.read()
            assert (m == tr.NO_HISTORY).all()
            assert lib.tri_taa_read(t._h, None, None, None) == abi.TRI_OK
            assert lib.tri_taa_get_output(t._h, None, None, None) == abi.TRI_OK
            assert code(lambda: t.blit(r, 0, 4)) == abi.TRI_E_INVALID
            r.set_motion_output(False)
            fails(lambda: t.resolve(r), abi.TRI_E_STATE, off)
        for w, hh in ((s.width + 1, s.height), (s.height, s.width)):  # another extent
            with open_raster(id_ref.cubes_and_quad(w, hh)) as other:
                other.render_frame()
                extent = f"the context is {w} x {hh}, the history {s.width} x {s.height}"
                fails(lambda: t.resolve(other), abi.TRI_E_INVALID, "tri_taa_resolve: " + extent)
                fails(lambda: t.blit(other, 8, 8), abi.TRI_E_INVALID, "tri_taa_blit_linear: " + extent)
        with open_raster(s, band=(16, 48)) as band:  # a row band
            band.render_frame()
            fails(lambda: t.resolve(band), abi.TRI_E_UNSUPPORTED, "tri_taa_resolve: a row-band context (the fetch and the 3 x 3 windows leave the band)")
            fails(lambda: t.blit(band, 8, 8), abi.TRI_E_STATE, "tri_taa_blit_linear: a row-band context has no whole frame")
        if torch.cuda.device_count() > 1:  # another device
            with open_raster(s, device=1) as far:
                far.render_frame()
                fails(lambda: t.resolve(far), abi.TRI_E_INVALID,
                      "tri_taa_resolve: the context is on device 1, the history on 0")


def test_images_blit_and_timing():
    import torch

    from trident_raster import abi, raster

    s = id_ref.sphere_and_quad()
    frames = chain_of(s, 2)
    with open_raster(s) as r, raster.TriTaa(s.width, s.height) as t:
        seen = []
        for k, (sc_, hist) in enumerate(frames):
            render(r, *jittered_frame(k, sc_, hist))
            t.resolve(r)
            col, acc, mask = t.images()
            assert (col.width, col.height, col.pitch_bytes, col.format) == (s.width, s.height, s.width * 4, abi.TRI_FORMAT_B8G8R8A8_UNORM)
            assert (acc.width, acc.height, acc.pitch_bytes, acc.format) == (s.width, s.height, s.width * 8, abi.TRI_FORMAT_R16G16B16A16_UNORM)
            assert (mask.width, mask.height, mask.pitch_bytes, mask.format) == (s.width, s.height, s.width, abi.TRI_FORMAT_R8_UINT)
            assert col.device_ptr and acc.device_ptr and mask.device_ptr and col.device == acc.device == mask.device == r.output_image().device
            assert col.device_ptr % 16 == 0 and acc.device_ptr % 16 == 0
            seen.append(acc.device_ptr)
            # colour16 is the set the last pass wrote: its bytes are tri_taa_read's rgba16
            res, a16, _ = t.read()
            n = s.width * s.height
            raw = raster.copy_device_to_host(acc.device_ptr, s.height * acc.pitch_bytes, acc.device)
            assert np.array_equal(raw.view(np.uint16).reshape(s.height, s.width, 4), a16)
            raw = raster.copy_device_to_host(col.device_ptr, s.height * col.pitch_bytes, col.device)
            assert np.array_equal(raw.reshape(s.height, s.width, 4), res)
        assert seen[0] != seen[1]  # the two sets alternate
        # the presentation blit at the frame's own extent is the resolved image
        t.blit(r, s.width, s.height)
        assert np.array_equal(r.read_present(), res)
        r.blit(s.width, s.height)
        assert np.array_equal(r.read_present(), snapshot(r)[2])  # ... and tri_blit_linear still shows the raw frame
        out = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        t.blit(r, s.width, s.height, out.data_ptr())
        r.synchronize()
        assert np.array_equal(out.cpu().numpy().view(np.uint8).reshape(s.height, s.width, 4), res)
        t.blit(r, 2 * s.width, s.height // 2)
        assert r.read_present().shape == (s.height // 2, 2 * s.width, 4)

        assert t.timing() == (0.0, 0)  # the context asked for no timed frame
        r.set_timing(True)
        for k in range(3):
            r.render()
            t.resolve(r)
            r.synchronize()
            assert t.timing()[1] == k + 1
        ms, passes = t.timing()
        tm = r.timing()
        print(f"TAA timing: {1e3 * ms / passes:.1f} us per pass in k_taa_resolve, stages {tm}")
        assert passes == 3 and ms > 0.0 and tm["frames"] == 3
        r.set_timing(False)
        r.render()
        t.resolve(r)
        assert t.timing() == (ms, 3)
