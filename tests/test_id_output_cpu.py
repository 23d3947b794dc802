"""CPU tests of the entity-id pass: the header and its Python mirror, the reference of tests/id_ref.py against frames
whose ids are known by construction, the argument errors that need no device, and `make id-check` (the plain-C++ rules
under the address and undefined-behaviour sanitizers)."""
import ctypes as C
import os
import subprocess

import numpy as np

import id_ref
from trident_raster import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tri_raster.h")
PKG = os.path.join(ROOT, "3d-renderer_amd")

ID_FUNCTIONS = ["tri_set_id_output", "tri_read_ids", "tri_get_id_output", "tri_pick", "tri_pick_rect", "tri_set_outline",
                "tri_get_id_timing",
                "tri_group_set_id_output", "tri_group_read_ids", "tri_group_pick"]


def test_header_and_mirror_agree():
    import re

    text = open(HEADER).read()
    declared = set(re.findall(r"^(?:int|const char\*|uint64_t)\s+(tri_\w+)\(", text, flags=re.M))
    mirrored = {n for n, _, _ in abi.CABI_FUNCTIONS}
    for name in ID_FUNCTIONS:
        assert name in declared and name in mirrored, name
    assert declared == mirrored
    assert re.search(r"#define TRI_FORMAT_R32_UINT 98u", text) and abi.TRI_FORMAT_R32_UINT == 98
    assert re.search(r"#define TRI_RASTER_ABI_VERSION 2\b", text) and abi.TRI_RASTER_ABI_VERSION == 2


def test_struct_sizes_match_the_c_compiler(tmp_path):
    structs = {"tri_pick_result": abi.TriPickResult, "tri_outline": abi.TriOutline}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.strip().splitlines())
    for cname, py in structs.items():
        assert int(out[f"{cname} size"]) == C.sizeof(py), cname
        for fname, _ in py._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(py, fname).offset, (cname, fname)
    assert C.sizeof(abi.TriPickResult) == 16 and C.sizeof(abi.TriOutline) == 40


def test_abi_version_and_exports(hiplib):
    assert hiplib.tri_abi_version() == 2
    out = subprocess.run(["nm", "-D", "--defined-only", hiplib._name], capture_output=True, text=True, check=True).stdout
    for name in ID_FUNCTIONS:
        assert f" T {name}\n" in out, name


def test_argument_errors_need_no_device(hiplib):
    """Null handles and null results are TRI_E_INVALID on every host, with the entry point named in the message."""
    pick = abi.TriPickResult()
    img = abi.TriImage()
    n = C.c_uint32()
    ms, frames = C.c_double(), C.c_uint64()
    bits = (C.c_uint32 * 1)()
    outline = abi.TriOutline()
    outline.width_px = 2
    calls = {
        "tri_set_id_output": lambda: hiplib.tri_set_id_output(None, 1),
        "tri_read_ids": lambda: hiplib.tri_read_ids(None, bits),
        "tri_get_id_output": lambda: hiplib.tri_get_id_output(None, C.byref(img)),
        "tri_pick": lambda: hiplib.tri_pick(None, 0, 0, C.byref(pick)),
        "tri_pick_rect": lambda: hiplib.tri_pick_rect(None, 0, 0, 1, 1, bits, 1, C.byref(n)),
        "tri_set_outline": lambda: hiplib.tri_set_outline(None, C.byref(outline)),
        "tri_get_id_timing": lambda: hiplib.tri_get_id_timing(None, C.byref(ms), C.byref(frames)),
        "tri_group_set_id_output": lambda: hiplib.tri_group_set_id_output(None, 1),
        "tri_group_read_ids": lambda: hiplib.tri_group_read_ids(None, bits),
        "tri_group_pick": lambda: hiplib.tri_group_pick(None, 0, 0, C.byref(pick)),
    }
    for name, call in calls.items():
        assert call() == abi.TRI_E_INVALID, name
        message = hiplib.tri_last_error()
        assert name.replace("tri_group_set_id_output", "tri_group").encode() in message, (name, message)


def test_reference_on_a_hand_made_frame():
    """ids_from_depths over depth images written by hand: quad A at 0.5, quad B at 0.25 over part of it, quad C
    coincident with B. C owns B's pixels (the last of the draws that reach the minimum), A the rest of its own."""
    w, h = 40, 24
    rects = id_ref.hand_made(w, h)
    singles = []
    full = np.full((h, w), id_ref.BG, np.uint32)
    for x0, y0, x1, y1, z in rects:
        d = np.full((h, w), id_ref.BG, np.uint32)
        d[y0:y1, x0:x1] = np.float32(z).view(np.uint32)
        singles.append(d)
        full = np.minimum(full, d)  # non-negative float bits order like the floats
    ids = id_ref.ids_from_depths(full, singles)
    want = np.zeros((h, w), np.uint32)
    want[3:20, 2:30] = 1
    want[1:12, 10:38] = 3
    assert np.array_equal(ids, want)
    assert np.array_equal(ids, id_ref.ids_of_rects(w, h, rects))
    assert 2 not in ids and set(np.unique(ids)) == {0, 1, 3}


def test_reference_through_the_oracle(oracle):
    """The same frame rendered by the oracle (full frame and one draw at a time), whole and as a row band."""
    w, h = 40, 24
    rects = id_ref.hand_made(w, h)
    scene = id_ref.pixel_quads("id_hand_made", w, h, rects)
    ids, depth = id_ref.expected_ids(oracle, scene)
    assert np.array_equal(ids, id_ref.ids_of_rects(w, h, rects))
    assert int((depth != id_ref.BG).sum()) == int((ids != 0).sum())
    band = (5, 18)
    bids, _ = id_ref.expected_ids(oracle, scene, band=band)
    assert np.array_equal(bids, ids[band[0]:band[1]])


def test_reference_keeps_the_callers_index_over_a_skipped_draw(oracle):
    scene = id_ref.with_skipped_draw(id_ref.cubes_and_quad())
    ids, _ = id_ref.expected_ids(oracle, scene)
    plain, _ = id_ref.expected_ids(oracle, id_ref.cubes_and_quad())
    assert 2 not in ids  # the skipped draw owns nothing
    shifted = plain.copy()
    shifted[plain >= 2] += 1
    assert np.array_equal(ids, shifted) and {1, 3, 4} <= set(np.unique(ids))


def test_outline_restatement():
    """outline_mask against the rule spelled out per pixel, at the widths the kernel supports and at the array's edges."""
    rng = np.random.default_rng(4)
    ids = np.zeros((19, 23), np.uint32)
    ids[0:4, 0:5] = 1      # touches two edges
    ids[8:11, 9:14] = 2
    ids[17:19, 20:23] = 3  # touches the other two
    ids[rng.integers(0, 19, 6), rng.integers(0, 23, 6)] = 2
    for r in (1, 3, 8):
        for selected in ([], [0], [1, 2], [0, 1, 2], [7]):
            got = id_ref.outline_mask(ids, selected, r)
            sel = np.isin(ids, [s + 1 for s in selected])
            want = np.zeros(ids.shape, bool)
            for y in range(ids.shape[0]):
                for x in range(ids.shape[1]):
                    if sel[y, x]:
                        continue
                    want[y, x] = sel[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1].any()
            assert np.array_equal(got, want), (r, selected)
    assert np.array_equal(id_ref.colour_bytes((1.0, 0.6, 0.0, 1.0)), np.array([0, 153, 255, 255], np.uint8))


def test_make_id_check_is_clean():
    """host/tools/id_check.cpp under -fsanitize=address,undefined: its own program, run on the CPU."""
    p = subprocess.run(["make", "-s", "-C", PKG, "id-check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "id_check ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
