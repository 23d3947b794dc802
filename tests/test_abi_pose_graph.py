"""CPU checks of the pose-graph boundary: the new records' layout against the C compiler, the exported symbols of both
libraries, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

from trident_raster import abi, app

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tri_raster.h")
NEW = ("tri_animset_add_mask", "tri_pose_graph", "tri_group_pose_graph")


def test_record_layouts_match_the_c_compiler(tmp_path):
    structs = {"tri_pose_op": (abi.TriPoseOp, abi.POSE_OP_DTYPE),
               "tri_pose_graph_instance": (abi.TriPoseGraphInstance, abi.POSE_GRAPH_INSTANCE_DTYPE)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, (py, _) in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in py._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    for name in ("TRI_POSE_STACK", "TRI_POSE_MAX_OPS", "TRI_POSE_NO_MASK", "TRI_POSE_OP_REST", "TRI_POSE_OP_CLIP",
                 "TRI_POSE_OP_BLEND", "TRI_POSE_OP_ADD"):
        lines.append(f'printf("{name} %llu\\n", (unsigned long long){name});')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-o", str(exe), str(src)], check=True)
    out = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.strip().splitlines())
    for cname, (py, dtype) in structs.items():
        assert int(out[f"{cname} size"]) == C.sizeof(py) == dtype.itemsize == 16, cname
        for fname, _ in py._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(py, fname).offset == dtype.fields[fname][1], (cname, fname)
    for name in ("TRI_POSE_STACK", "TRI_POSE_MAX_OPS", "TRI_POSE_NO_MASK", "TRI_POSE_OP_REST", "TRI_POSE_OP_CLIP",
                 "TRI_POSE_OP_BLEND", "TRI_POSE_OP_ADD"):
        assert int(out[name]) == getattr(abi, name), name


def test_both_libraries_export_the_new_symbols(hiplib):
    out = subprocess.run(["nm", "-D", "--defined-only", hiplib._name], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (tri_\w+)", out))
    assert set(NEW) <= exported
    assert set(NEW) <= {n for n, _, _ in abi.CABI_FUNCTIONS}
    shim = app.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", shim._name], capture_output=True, text=True, check=True).stdout
    assert "trident_anim_eval_program" in set(re.findall(r"\bT (trident_\w+)", out))


def test_null_arguments_are_refused_without_a_device(hiplib):
    inst = (abi.TriPoseGraphInstance * 1)()
    ops = (abi.TriPoseOp * 1)()
    mask = C.c_uint32()
    assert hiplib.tri_pose_graph(None, None, inst, 1, ops, 1) == abi.TRI_E_INVALID
    assert hiplib.tri_group_pose_graph(None, None, inst, 1, ops, 1) == abi.TRI_E_INVALID
    assert hiplib.tri_animset_add_mask(None, 0, None, 0, C.byref(mask)) == abi.TRI_E_INVALID
    assert b"tri_animset_add_mask" in hiplib.tri_last_error()
