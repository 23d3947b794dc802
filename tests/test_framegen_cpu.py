"""The frame generator without a GPU: the exporter and the weights container, the parser's refusals through the shim,
the model path search, the statistics without a model, the ABI mirror, and the stand-alone sanitizer check."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import framegen_ref
from trident_raster import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import export_frame_generator as exporter  # noqa: E402

NEW_ENTRY_POINTS = ["tri_nn_pack_weights", "tri_nn_conv", "tri_framegen_create", "tri_framegen_destroy", "tri_framegen_info",
                    "tri_framegen_submit", "tri_framegen_poll", "tri_framegen_wait", "tri_framegen_output",
                    "tri_framegen_read_output", "tri_framegen_last_ms", "tri_upload_ai_frame_device", "tri_read_ai_frame",
                    "tri_get_stream"]


@pytest.fixture(scope="module")
def state():
    return framegen_ref.make_state(4, 321)


@pytest.fixture(scope="module")
def good(state):
    blob = framegen_ref.container_bytes(state, 4)
    return blob


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


def _entry(blob, name):
    count = struct.unpack_from("<I", blob, 16)[0]
    for i in range(count):
        at = framegen_ref.HEADER_BYTES + framegen_ref.ENTRY_BYTES * i
        if blob[at:at + 64].rstrip(b"\0") == name.encode():
            return at
    raise KeyError(name)


@pytest.mark.parametrize("wrapped", [True, False])
def test_exporter_round_trips_a_checkpoint(tmp_path, state, good, wrapped):
    """torch.save wrote {"model_state": ...} or a bare state_dict; the tool copies the named float tensors."""
    ckpt, out = tmp_path / "gen.pt", tmp_path / "frame_generator.trifgen"
    torch.save({"model_state": state, "epoch": 3} if wrapped else state, ckpt)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "export_frame_generator.py"), str(ckpt), str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blob = out.read_bytes()
    assert blob == good  # the tool and the tests' own writer agree byte for byte
    channels, tensors = exporter.read_container(blob)
    floats = {k: v for k, v in state.items() if v.is_floating_point()}
    assert channels == 4 and sorted(tensors) == sorted(floats)
    assert not any(k.endswith("num_batches_tracked") for k in tensors)
    for k, v in floats.items():
        assert tensors[k].dtype == np.float32 and np.array_equal(tensors[k].view(np.uint32), v.numpy().view(np.uint32)), k


def test_pack_weights_layouts(hiplib):
    """tri_nn_pack_weights (host only): [ky][kx][ci][co], and for the transposed convolution
    [py][px][a][b][ci][co] with ky = 1 - py + 2a, kx = 1 - px + 2b — no flip."""
    from trident_raster import raster

    w = np.arange(7 * 5 * 9, dtype=np.float32).reshape(7, 5, 3, 3)  # [co][ci][ky][kx]
    p = raster.nn_pack_weights(abi.TriNnConvDesc(abi.TRI_NN_CONV3X3, 1, 4, 4, 5, 7, 0, 0), w).reshape(3, 3, 5, 7)
    assert np.array_equal(p, w.transpose(2, 3, 1, 0))
    wt = np.arange(5 * 7 * 16, dtype=np.float32).reshape(5, 7, 4, 4)  # [ci][co][ky][kx]
    p = raster.nn_pack_weights(abi.TriNnConvDesc(abi.TRI_NN_CONVT4X4, 2, 4, 4, 5, 7, 0, 0), wt).reshape(2, 2, 2, 2, 5, 7)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    assert np.array_equal(p[py, px, a, b], wt[:, :, 1 - py + 2 * a, 1 - px + 2 * b])


def _damaged(good, state):
    """name -> (bytes, what the message must name)."""
    victim = "m_EncoderStage3.2.m_Block.0.weight"
    var = "m_DecodeStage1.2.m_Block.1.running_var"
    e = _entry(good, victim)

    def patched(at, fmt, *values):
        b = bytearray(good)
        struct.pack_into(fmt, b, at, *values)
        return bytes(b)

    var_at = struct.unpack_from("<Q", good, _entry(good, var) + 88)[0]
    offset = struct.unpack_from("<Q", good, e + 88)[0]
    return {
        "truncated": (good[:len(good) - 1], "truncated"),
        "truncated table": (good[:1000], "truncated"),
        "oversized dimension": (patched(e + 68, "<I", 0x80000000), victim),
        "missing tensor": (framegen_ref.container_bytes(state, 4, skip=(victim,)), victim),
        "wrong shape": (patched(e + 72, "<I", 64), victim),
        "misaligned offset": (patched(e + 88, "<Q", offset + 2), victim),
        "NaN variance": (patched(var_at + 8, "<f", float("nan")), var),
        "wrong magic": (b"TRIFGEM\0" + good[8:], "magic"),
    }


def test_parser_refusals_go_through_the_shim(app_mod, tmp_path, state, good):
    a = app_mod.TridentApp()
    from trident_raster.raster import TriError

    for name, (blob, needle) in _damaged(good, state).items():
        path = tmp_path / (name.replace(" ", "_") + ".trifgen")
        path.write_bytes(blob)
        with pytest.raises(TriError) as e:
            a.load_ai_model(path)
        assert e.value.code == abi.TRI_E_INVALID, name
        assert needle in str(e.value), (name, str(e.value))
        assert a.ai_model_info()[0] is False
    with pytest.raises(TriError) as e:
        a.load_ai_model(tmp_path / "absent.trifgen")
    assert e.value.code == abi.TRI_E_INVALID and "cannot open" in str(e.value)
    # a good one loads without a device: the device generator is made for the first frame's extent
    path = tmp_path / "good.trifgen"
    path.write_bytes(good)
    a.load_ai_model(path)
    assert a.ai_model_info() == (True, [1, -1, -1, 4], [1, -1, -1, 3])
    assert a.ai_readback_enabled()  # an initialised generator needs the readback (Renderer.cpp:787)
    # a damaged file named afterwards is refused and the loaded model stays
    with pytest.raises(TriError):
        a.load_ai_model(tmp_path / "truncated.trifgen")
    assert a.ai_model_info()[0] is True
    a.close()


def test_parser_refusals_in_the_library(hiplib, state, good):
    """tri_framegen_create parses before it asks for a device: TRI_E_INVALID with the tensor's name on every host."""
    for name, (blob, needle) in _damaged(good, state).items():
        handle = C.c_void_p(1)
        assert hiplib.tri_framegen_create(-1, blob, len(blob), 64, 48, C.byref(handle)) == abi.TRI_E_INVALID, name
        assert needle.encode() in hiplib.tri_last_error() and not handle.value, (name, hiplib.tri_last_error())
    handle = C.c_void_p(1)
    assert hiplib.tri_framegen_create(-1, good, len(good), 6, 8, C.byref(handle)) == abi.TRI_E_INVALID
    assert hiplib.tri_framegen_create(-1, good, len(good), 0, 8, C.byref(handle)) == abi.TRI_E_INVALID
    assert hiplib.tri_framegen_create(-1, None, 0, 8, 8, C.byref(handle)) == abi.TRI_E_INVALID


def test_debug_stats_without_a_model_read_zero(app_mod):
    a = app_mod.TridentApp()
    stats = a.ai_debug_stats()
    assert set(stats) == {"model_initialised", "pending_job_count", "completed_inference_count", "last_inference_ms",
                          "average_inference_ms", "texture_ready", "blend_strength", "texture_width", "texture_height",
                          "reserved_metric"}
    assert all(v == 0 for v in stats.values()), stats
    assert a.ai_model_info() == (False, [0, 0, 0, 0], [0, 0, 0, 0])
    assert a.finish_ai_inference(0) is True  # no job in flight
    assert a.read_ai_blend_frame() is None
    a.close()


def test_model_path_search_order(app_mod, tmp_path, monkeypatch, good):
    """TRIDENT_AI_MODEL first (when the file exists), then Assets/AI/frame_generator.trifgen under the working
    directory, its parent and its grandparent (Renderer.cpp:1743-1782)."""
    a = app_mod.TridentApp()
    deep = tmp_path / "top" / "mid" / "cwd"
    deep.mkdir(parents=True)
    monkeypatch.chdir(deep)
    monkeypatch.delenv("TRIDENT_AI_MODEL", raising=False)

    def model_under(root):
        p = root / "Assets" / "AI" / "frame_generator.trifgen"
        p.parent.mkdir(parents=True)
        p.write_bytes(good)
        return os.path.realpath(p)

    def resolved():
        p = a.resolve_ai_model_path()
        return None if p is None else os.path.realpath(p)

    assert resolved() is None
    assert a.try_initialise_ai_model() is False
    beyond = model_under(tmp_path)  # the great-grandparent is not searched
    assert resolved() is None
    top = model_under(tmp_path / "top")
    assert resolved() == top
    mid = model_under(tmp_path / "top" / "mid")
    assert resolved() == mid
    here = model_under(deep)
    assert resolved() == here
    named = tmp_path / "named.trifgen"
    monkeypatch.setenv("TRIDENT_AI_MODEL", str(named))
    assert resolved() == here  # the variable names no file: the default search
    named.write_bytes(good)
    assert resolved() == os.path.realpath(named)
    monkeypatch.setenv("TRIDENT_AI_MODEL", "")
    assert resolved() == here
    assert beyond != here and a.try_initialise_ai_model() is True and a.ai_model_info()[0] is True
    a.close()


def test_abi_mirror_lists_the_new_entry_points(hiplib):
    text = open(os.path.join(ROOT, "include", "tri_raster.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*|uint64_t)\s+(tri_\w+)\(", text, flags=re.M))
    mirrored = {n for n, _, _ in abi.CABI_FUNCTIONS}
    assert declared == mirrored
    assert set(NEW_ENTRY_POINTS) <= mirrored
    out = subprocess.run(["nm", "-D", "--defined-only", hiplib._name], capture_output=True, text=True, check=True).stdout
    assert set(NEW_ENTRY_POINTS) <= set(re.findall(r"\bT (tri_\w+)", out))
    assert hiplib.tri_abi_version() == 2
    assert C.sizeof(abi.TriNnConvDesc) == 32


def test_make_framegen_check():
    """The parser, the BatchNorm fold and the re-lay over a good container and damaged copies of it, as a stand-alone
    program under the address and undefined-behaviour sanitizers (nothing is loaded into Python)."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "3d-renderer_amd"), "framegen-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "framegen_check ok" in r.stdout
