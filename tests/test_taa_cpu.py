"""CPU tests of temporal anti-aliasing: `make taa-check` (the rule the kernel compiles, under the address and
undefined-behaviour sanitizers), the jitter against float64, the rule's restatement (tests/taa_ref.py) through the oracle
under jittered projections — how much of a silhouette's error it removes, and what two wrong rules do instead — the header
and its Python mirror, and the argument errors that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import id_ref
import motion_ref as mr
import taa_ref as tr
from trident_raster import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tri_raster.h")
PKG = os.path.join(ROOT, "3d-renderer_amd")
F = np.float32

TAA_FUNCTIONS = ["tri_taa_jitter", "tri_taa_jitter_projection", "tri_taa_create", "tri_taa_destroy", "tri_taa_resolve",
                 "tri_taa_reset", "tri_taa_read", "tri_taa_get_output", "tri_taa_get_timing", "tri_taa_blit_linear"]
PERIOD, ALPHA = 8, 0.1
EDGE_DEG = 20.0  # the silhouette's angle in the quality run (DESIGN 5p records the measured ratio)


def test_make_taa_check_is_clean():
    """host/tools/taa_check.cpp under -fsanitize=address,undefined: its own program, run on the CPU."""
    p = subprocess.run(["make", "-s", "-C", PKG, "taa-check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr


# ---- the jitter -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [0, 1, 8, 16, 64])
def test_jitter_is_the_centred_halton_point(hiplib, period):
    from trident_raster import raster

    for index in list(range(2 * max(period, 1) + 3)) + [1000, 0xFFFFFFFF]:
        x, y = raster.taa_jitter(index, period)
        wx, wy = tr.jitter(index, period)
        assert x == F(wx) and y == F(wy), (index, period)
        assert -0.5 <= x < 0.5 and -0.5 <= y < 0.5
    if period:
        pts = {raster.taa_jitter(k, period) for k in range(period)}
        assert len(pts) == period  # distinct sub-pixel positions
    else:
        assert raster.taa_jitter(7, 0) == (0.0, 0.0)


def test_jitter_refuses_a_period_above_64(hiplib):
    xy = (C.c_float * 2)()
    assert hiplib.tri_taa_jitter(0, 65, C.byref(xy)) == abi.TRI_E_INVALID and b"tri_taa_jitter" in hiplib.tri_last_error()
    assert hiplib.tri_taa_jitter(0, 64, C.byref(xy)) == abi.TRI_OK
    assert hiplib.tri_taa_jitter(0, 8, None) == abi.TRI_E_INVALID


def cameras(w, h):
    """A perspective and an orthographic projection (column-major float32 [16]) with a view each."""
    from trident_raster import scenes

    view, proj = scenes.editor_camera((0.3, -0.2, 5.0), (5.0, -8.0, 2.0), 60.0, (w, h), 0.1, 60.0)
    ortho = np.zeros((4, 4), np.float64)  # mathematical: x in -4..4, y in -3..3 (y down), z 0.1..60 -> 0..1
    ortho[0, 0], ortho[1, 1], ortho[2, 2], ortho[2, 3], ortho[3, 3] = 2.0 / 8.0, -2.0 / 6.0, -1.0 / 59.9, -0.1 / 59.9, 1.0
    return {"perspective": (np.asarray(view, F).reshape(16), np.asarray(proj, F).reshape(16)),
            "orthographic": (np.asarray(view, F).reshape(16), mr.to_cm(ortho).reshape(16))}


def project_f64(view, proj, pts, w, h):
    """World points [n, 3] -> (pixel x, pixel y, depth), float64, under the pixel convention of the motion pass."""
    clip = mr.mat(proj) @ mr.mat(view) @ np.concatenate([pts, np.ones((len(pts), 1))], axis=1).T
    assert (clip[3] > 0).all()
    return (clip[0] / clip[3] + 1.0) * 0.5 * w, (clip[1] / clip[3] + 1.0) * 0.5 * h, clip[2] / clip[3]


@pytest.mark.parametrize("w,h", [(37, 23), (3840, 2160)])
@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
def test_jittered_projection_moves_every_point_by_the_jitter(hiplib, kind, w, h):
    from trident_raster import raster

    view, proj = cameras(w, h)[kind]
    rng = np.random.default_rng(w + len(kind))
    pts = rng.uniform((-2.0, -1.5, -3.0), (2.0, 1.5, 2.0), (200, 3))
    x0, y0, z0 = project_f64(view, proj, pts, w, h)
    worst = 0.0
    for index in range(8):
        jx, jy = raster.taa_jitter(index, 8)
        got = raster.taa_jitter_projection(proj, jx, jy, w, h)
        # the specification itself, in float64 and rounded once
        assert np.array_equal(got, tr.jitter_projection(proj, jx, jy, w, h).astype(F))
        assert np.array_equal(got.reshape(4, 4)[:, 2:].view(np.uint32), proj.reshape(4, 4)[:, 2:].view(np.uint32))  # rows 2, 3
        x, y, z = project_f64(view, got, pts, w, h)
        worst = max(worst, float(np.abs(x - x0 - float(jx)).max()), float(np.abs(y - y0 - float(jy)).max()))
        assert np.array_equal(z, z0)  # depth unchanged, to the bit
    print(f"TAA jitter {kind} {w} x {h}: worst |move - jitter| {worst:.3e} px")
    assert worst <= 1e-4


def test_same_jitter_on_both_projections_gives_identity_rows(hiplib):
    """The contract's still case: a jittered current and a same-jitter previous projection are bitwise equal."""
    from trident_raster import raster

    s = id_ref.cubes_and_quad()
    for index in range(8):
        jx, jy = raster.taa_jitter(index, 8)
        cur = tr.jittered(s, jx, jy)
        hist = tr.contract_history(s, jx, jy)
        table = raster.motion_matrices(cur.ubo, cur.draws, hist)
        assert np.array_equal(table.view(np.uint32), np.broadcast_to(np.eye(4, dtype=F), table.shape).view(np.uint32)), index
    # ... and an unjittered previous projection under a jittered current one does not
    jx, jy = raster.taa_jitter(1, 8)
    cur = tr.jittered(s, jx, jy)
    table = raster.motion_matrices(cur.ubo, cur.draws, (*mr.camera_of(s.ubo), None))
    assert not np.array_equal(table[0], np.eye(4, dtype=F))


# ---- quality: a static slanted silhouette through the oracle ----------------------------------------------------------------
def edge_scene(w=64, h=48, angle=EDGE_DEG):
    """One bright quad whose left edge crosses the whole frame at `angle` from the vertical, over the dark clear
    colour; its other edges lie outside the frame."""
    from trident_raster import scenes

    qv, qi = id_ref.quad_mesh()
    s = id_ref.mesh_scene("taa_edge", w, h, [(qv, qi, scenes.compose_transform((3.2, 0.0, 0.0), (0.0, 0.0, angle), (3.0, 12.0, 1.0)))])
    # ambient light alone: the quad is one flat colour, so only the silhouette is "not constant"
    s.ubo.light_counts = (abi.C.c_uint32 * 4)(0, 0, 0, 0)
    s.ubo.ambient_color_intensity = (abi.C.c_float * 4)(1.0, 1.0, 1.0, 3.0)
    return s


def oracle_frame(oracle, scene):
    """(colour, ids, depth bits) of a one-draw scene through the oracle."""
    col, dep = oracle.render(scene)[:2]
    return col, (dep != id_ref.BG).astype(np.uint32), dep


_STATIC = {}


def static_run(oracle, frames=40):
    """The static edge scene: the unjittered frame, the truth (the mean of an 8 x 8 sub-pixel grid of jittered oracle
    frames), and `frames` jittered frames restated by the rule and by the nearest-id mutant. Computed once, shared,
    never modified."""
    from trident_raster import raster

    if not _STATIC:
        s = edge_scene()
        raw = oracle_frame(oracle, s)[0]
        grid = [(i + 0.5) / 8.0 - 0.5 for i in range(8)]
        truth = np.mean([oracle_frame(oracle, tr.jittered(s, jx, jy))[0].astype(np.float64) for jy in grid for jx in grid], axis=0)
        rule, mutant = [], []
        prev = prev_m = None
        for n in range(frames):
            jx, jy = raster.taa_jitter(n, PERIOD)
            cur = tr.jittered(s, jx, jy)
            col, ids, dep = oracle_frame(oracle, cur)
            table = raster.motion_matrices(cur.ubo, cur.draws, tr.contract_history(s, jx, jy))
            acc, res, mask = tr.restate(table, ids, dep, col, prev, s.width, s.height, ALPHA)
            prev = (acc, ids)
            rule.append((res, mask, col))
            acc, res, mask = tr.restate(table, ids, dep, col, prev_m, s.width, s.height, ALPHA, id_test="nearest")
            prev_m = (acc, ids)
            mutant.append((res, mask))
        for a in [raw, truth] + [x for f in rule + mutant for x in f]:
            a.setflags(write=False)
        _STATIC.update(raw=raw, truth=truth, rule=rule, mutant=mutant, edge=tr.silhouette(raw), flat=tr.flat5(raw))
    return _STATIC


def edge_error(img, st):
    return float(np.abs(img[..., :3].astype(np.float64) - st["truth"][..., :3])[st["edge"]].mean())


def test_the_resolved_silhouette_halves_the_raw_error(oracle, hiplib):
    st = static_run(oracle)
    e0 = edge_error(st["raw"], st)
    errs = [edge_error(res, st) for res, _, _ in st["rule"]]
    print(f"TAA quality: {int(st['edge'].sum())} silhouette pixels, raw error E0 {e0:.2f} LSB; resolved, frames 32..39: "
          + " ".join(f"{e:.2f}" for e in errs[32:40]) + f"; worst ratio {max(errs[32:40]) / e0:.3f}")
    assert st["edge"].sum() >= 48 and e0 > 4.0  # a high-contrast silhouette across the frame
    for n in range(32, 32 + PERIOD):
        assert errs[n] <= 0.5 * e0, (n, errs[n], e0)


def test_flat_pixels_stay_exact_and_nothing_is_clamped(oracle, hiplib):
    st = static_run(oracle)
    assert st["flat"].sum() > 0.5 * st["flat"].size
    assert (st["rule"][0][1] == tr.NO_HISTORY).all()
    for n, (res, mask, _) in enumerate(st["rule"]):
        assert np.array_equal(res[st["flat"]], st["raw"][st["flat"]]), n
        assert not (mask & tr.CLAMPED).any(), n
        if n:
            assert (mask == 0).all(), n  # a still scene: every pixel valid, the 3 x 3 id test included


def test_a_nearest_pixel_id_test_rejects_the_silhouette(oracle, hiplib):
    """The mutant sets ID on silhouette pixels of the static jittered run — the pixels that need accumulating — and the
    rule on none."""
    st = static_run(oracle)
    n_edge = int(st["edge"].sum())
    ids_set, most = 0, 0
    for n in range(32, 32 + PERIOD):
        (res, mask, _), (mres, mmask) = st["rule"][n], st["mutant"][n]
        rejected = (mmask & tr.ID) != 0
        differs = int(((mres != res).any(axis=-1) | (mmask != mask))[st["edge"]].sum())
        print(f"TAA nearest-id mutant, frame {n}: ID on {int(rejected.sum())} pixels ({int((rejected & st['edge']).sum())} on the "
              f"silhouette), differs from the rule on {differs} of {n_edge} silhouette pixels")
        assert not (mask & tr.ID).any()
        assert not (rejected & ~st["edge"]).any()
        ids_set += int(rejected.sum())
        most = max(most, differs)
    assert ids_set > 0
    assert most > 0.01 * n_edge


# ---- the clamp: a quad moving 3 px per frame ---------------------------------------------------------------------------------
def moving_quad(n, w=100, h=70):
    """Frame n of a bright quad that moves 3 px to the right per frame over the clear colour: (scene, motion history,
    ids by construction)."""
    rect = (10 + 3 * n, 20, 30 + 3 * n, 50, 0.5)
    s = id_ref.pixel_quads("taa_moving_quad", w, h, [rect])
    v, p = mr.camera_of(s.ubo)
    prev = np.array([mr.to_cm(mr.rigid((-3.0, 0.0, 0.0))).reshape(16)], F)  # it stood 3 px to the left
    return s, (v, p, prev), id_ref.ids_of_rects(w, h, [rect])


def test_without_the_clamp_a_moving_quad_leaves_a_trail(oracle, hiplib):
    """No id test here (it would reject the uncovered pixels by itself): the clamp alone has to remove stale history.
    Behind the quad: pixels it covered in an earlier frame, now background, whose 3 x 3 neighbourhood holds no quad pixel
    (next to the quad the neighbourhood's range contains the quad's colour, and clamping to it changes nothing — by the
    rule). There the rule gives the current frame exactly: the range is one colour. The mutant keeps 0.9^k of the quad."""
    from trident_raster import raster

    prev = prev_m = None
    covered = None
    for n in range(8):
        s, hist, want_ids = moving_quad(n)
        col, ids, dep = oracle_frame(oracle, s)
        assert np.array_equal(ids, want_ids)
        table = raster.motion_matrices(s.ubo, s.draws, hist if n else None)
        acc, res, mask = tr.restate(table, ids, dep, col, prev, s.width, s.height, ALPHA, reject_ids=False)
        prev = (acc, ids)
        macc, mres, mmask = tr.restate(table, ids, dep, col, prev_m, s.width, s.height, ALPHA, reject_ids=False, clamp=False)
        prev_m = (macc, ids)
        covered = (ids != 0) if covered is None else covered | (ids != 0)
    behind = covered & ~tr.window(ids != 0, np.logical_or)
    far = lambda img: (np.abs(img.astype(np.int32) - col.astype(np.int32)) > 2).any(axis=-1)  # noqa: E731
    edge = tr.silhouette(col)
    differs = int(((mres != res).any(axis=-1)).sum())
    print(f"TAA no-clamp mutant after 8 frames: {int(behind.sum())} pixels behind the quad, more than 2 LSB from the current "
          f"frame: rule {int(far(res)[behind].sum())}, mutant {int(far(mres)[behind].sum())}; CLAMPED on {int((mask & tr.CLAMPED != 0).sum())}; "
          f"the mutant differs on {differs} pixels, the silhouette has {int(edge.sum())}")
    assert behind.sum() >= 3 * 30 * 6  # 3 px x 30 rows per frame, less the column next to the quad
    assert not far(res)[behind].any()
    assert far(mres)[behind].sum() > 0.5 * behind.sum()
    assert (mask[behind] & tr.CLAMPED).any() and not (mmask & tr.CLAMPED).any()
    assert differs > 0.01 * edge.sum()
    assert (mask[ids != 0] & 15 == 0).all()  # the quad's own pixels follow it: valid history


# ---- header, mirror, exports, arguments ---------------------------------------------------------------------------------------
def test_header_and_mirror_agree():
    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|const char\*|uint64_t)\s+(tri_\w+)\(", text, flags=re.M))
    mirrored = {n for n, _, _ in abi.CABI_FUNCTIONS}
    for name in TAA_FUNCTIONS:
        assert name in declared and name in mirrored, name
    assert re.search(r"#define TRI_FORMAT_R16G16B16A16_UNORM 91u", text) and abi.TRI_FORMAT_R16G16B16A16_UNORM == 91
    assert re.search(r"#define TRI_TAA_REDO 1u", text) and abi.TRI_TAA_REDO == 1
    assert re.search(r"#define TRI_TAA_REJECT_ID 2u", text) and abi.TRI_TAA_REJECT_ID == 2
    for name, bit in [("NO_HISTORY", 1), ("NO_PROJ", 2), ("OUTSIDE", 4), ("ID", 8), ("CLAMPED", 32)]:
        assert re.search(rf"#define TRI_TAA_{name} {bit}u", text) and getattr(abi, f"TRI_TAA_{name}") == bit
        assert getattr(tr, name) == bit
    assert re.search(r"#define TRI_RASTER_ABI_VERSION 2\b", text) and abi.TRI_RASTER_ABI_VERSION == 2


def test_struct_layout_matches_the_c_compiler(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(tri_taa_params));']
    for fname, _ in abi.TriTaaParams._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(tri_taa_params, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.strip().splitlines())
    assert int(out["size"]) == C.sizeof(abi.TriTaaParams) == 16
    for fname, _ in abi.TriTaaParams._fields_:
        assert int(out[fname]) == getattr(abi.TriTaaParams, fname).offset, fname


def test_exports(hiplib):
    assert hiplib.tri_abi_version() == 2
    out = subprocess.run(["nm", "-D", "--defined-only", hiplib._name], capture_output=True, text=True, check=True).stdout
    for name in TAA_FUNCTIONS:
        assert f" T {name}\n" in out, name


def test_argument_errors_need_no_device(hiplib):
    img = abi.TriImage()
    ms, n = C.c_double(), C.c_uint64()
    buf = (C.c_uint8 * 64)()
    params = abi.TriTaaParams(0.1, 0)
    h = C.c_void_p()
    m = (C.c_float * 16)()
    calls = {
        "tri_taa_create": lambda: hiplib.tri_taa_create(-1, 16, 16, None),
        "tri_taa_resolve": lambda: hiplib.tri_taa_resolve(None, None, C.byref(params)),
        "tri_taa_reset": lambda: hiplib.tri_taa_reset(None),
        "tri_taa_read": lambda: hiplib.tri_taa_read(None, buf, buf, buf),
        "tri_taa_get_output": lambda: hiplib.tri_taa_get_output(None, C.byref(img), C.byref(img), C.byref(img)),
        "tri_taa_get_timing": lambda: hiplib.tri_taa_get_timing(None, C.byref(ms), C.byref(n)),
        "tri_taa_blit_linear": lambda: hiplib.tri_taa_blit_linear(None, None, None, 16, 16),
        "tri_taa_jitter_projection": lambda: hiplib.tri_taa_jitter_projection(None, 0.0, 0.0, 16, 16, C.byref(m)),
    }
    for name, call in calls.items():
        assert call() == abi.TRI_E_INVALID, name
        assert name.encode() in hiplib.tri_last_error(), name
    assert hiplib.tri_taa_jitter_projection(C.byref(m), 0.0, 0.0, 0, 16, C.byref(m)) == abi.TRI_E_INVALID
    # the extent rules come before any device is looked for
    for w, hh in [(0, 16), (16, 0), (0, 0), (65536, 32769), (0xFFFFFFFF, 0xFFFFFFFF)]:
        assert hiplib.tri_taa_create(-1, w, hh, C.byref(h)) == abi.TRI_E_INVALID, (w, hh)
        assert b"tri_taa_create" in hiplib.tri_last_error() and not h.value
    assert hiplib.tri_taa_destroy(None) == abi.TRI_OK
