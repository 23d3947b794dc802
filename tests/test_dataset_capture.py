"""AI readback and dataset capture, the host side (no GPU): the exported symbols, Trident::FrameDatasetRecorder's
files against the numpy restatement (tests/tensor_ref.py) byte for byte, its interval / index / pairing rules, the
AI output normalisation bit for bit, and the environment variables Renderer::Init honours."""
import ctypes as C
import os

import numpy as np
import pytest

import tensor_ref


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


@pytest.fixture()
def rec(app_mod, tmp_path):
    r = app_mod.DatasetRecorder()
    r.set_directory(tmp_path / "cap")
    yield r
    r.close()


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_restatement_pins():
    """Guards the yardstick: the constant, 255 -> 1.0f exactly, and how often a division would differ."""
    t = tensor_ref.unorm_table()
    assert t.dtype == np.float32 and t[0] == 0.0 and t[255] == np.float32(1.0)
    assert int(_bits(t)[1]) == 0x3B808081
    div = tensor_ref.division_variant(np.arange(256))
    assert int((_bits(t) != _bits(div)).sum()) == 126
    px = np.array([[10, 20, 30, 40]], np.uint8)  # B, G, R, A in memory
    assert np.array_equal(tensor_ref.tensor_from_bgra(px), t[[30, 20, 10, 40]][None])


def test_new_symbols_are_exported(hiplib, app_mod):
    from trident_raster import abi

    names = {n for n, _, _ in abi.CABI_FUNCTIONS}
    cabi = {"tri_convert_rgba_f32", "tri_framegrab_create", "tri_framegrab_destroy", "tri_framegrab_capture",
            "tri_framegrab_wait", "tri_framegrab_release"}
    assert cabi <= names
    for n in cabi:
        assert getattr(hiplib, n)
    assert hiplib.tri_abi_version() == 2
    assert abi.TRI_GRAB_HOST_COPY == 1
    lib = app_mod.load_library()
    for n in ["trident_app_set_dataset_capture", "trident_app_dataset_capture_state", "trident_app_set_ai_readback",
              "trident_app_ai_readback_state", "trident_app_acquire_frame", "trident_app_readback_device_tensor",
              "trident_app_submit_ai_output", "trident_ai_normalise_output", "trident_dataset_create",
              "trident_dataset_destroy", "trident_dataset_set_directory", "trident_dataset_set_interval",
              "trident_dataset_enable", "trident_dataset_reset", "trident_dataset_record_input",
              "trident_dataset_record_output", "trident_dataset_flush", "trident_dataset_state",
              "trident_dataset_write_npy"]:
        assert getattr(lib, n)


def test_cabi_argument_checks_need_no_device(hiplib):
    from trident_raster import abi

    fake = C.c_void_p(0x1000)  # never dereferenced: every call below fails its argument check
    call = hiplib.tri_convert_rgba_f32
    assert call(None, 4, 4, 16, fake, None) == abi.TRI_E_INVALID
    assert call(fake, 4, 4, 16, None, None) == abi.TRI_E_INVALID
    assert call(fake, 0, 4, 16, fake, None) == abi.TRI_E_INVALID
    assert call(fake, 4, 8193, 16, fake, None) == abi.TRI_E_INVALID
    assert call(fake, 4, 4, 12, fake, None) == abi.TRI_E_INVALID
    assert call(fake, 4, 4, 18, fake, None) == abi.TRI_E_INVALID
    assert call(C.c_void_p(0x1002), 4, 4, 16, fake, None) == abi.TRI_E_INVALID
    assert call(fake, 4, 4, 16, C.c_void_p(0x1002), None) == abi.TRI_E_INVALID
    assert hiplib.tri_last_error()
    out = C.c_void_p()
    assert hiplib.tri_framegrab_create(-1, 4, 4, 0, 0, C.byref(out)) == abi.TRI_E_INVALID
    assert hiplib.tri_framegrab_create(-1, 4, 4, 9, 0, C.byref(out)) == abi.TRI_E_INVALID
    assert hiplib.tri_framegrab_create(-1, 0, 4, 2, 0, C.byref(out)) == abi.TRI_E_INVALID
    assert hiplib.tri_framegrab_create(-1, 4, 4, 2, 2, C.byref(out)) == abi.TRI_E_INVALID  # an unknown flag
    assert not out.value
    assert hiplib.tri_framegrab_destroy(None) == abi.TRI_OK
    assert hiplib.tri_framegrab_capture(None, 0, None) == abi.TRI_E_INVALID
    assert hiplib.tri_framegrab_wait(None, 0, None, None) == abi.TRI_E_INVALID
    assert hiplib.tri_framegrab_release(None, 0) == abi.TRI_E_INVALID


# shape strings of 4 .. 19 characters: the header text lands on every residue of the 16-byte padding; ranks 1, 3, 4
# (and one of rank 6 for the longest)
_SHAPES = [(1,), (12,), (123,), (1234,), (12345,), (2, 3, 4), (11, 2, 3), (11, 12, 3), (1, 3, 5, 4), (1, 13, 5, 4),
           (1, 48, 64, 4), (1, 48, 64, 10), (1, 100, 64, 10), (1, 100, 640, 10), (1, 1080, 1920, 4), (1, 2, 3, 4, 5, 10)]


def test_npy_shapes_cover_every_padding_residue():
    residues = {(10 + len("{'descr': '<f4', 'fortran_order': False, 'shape': " + tensor_ref.shape_string(s) + ", }") + 1) % 16
                for s in _SHAPES}
    assert residues == set(range(16))
    assert {len(s) for s in _SHAPES} >= {1, 3, 4}


@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_npy_bytes_match_the_restatement(app_mod, tmp_path, shape):
    n = int(np.prod(shape))
    rng = np.random.default_rng(n)
    data = rng.random(n, dtype=np.float32)
    data[0] = np.float32(-0.0)
    path = tmp_path / "t.npy"
    assert app_mod.write_npy(path, data, shape)
    raw = path.read_bytes()
    assert raw == tensor_ref.npy_bytes(data, shape)
    assert (len(raw) - 4 * n) % 16 == 0 and raw[len(raw) - 4 * n - 1:len(raw) - 4 * n] == b"\n"
    back = np.load(path)
    assert back.dtype == np.float32 and back.shape == tuple(shape)
    assert np.array_equal(_bits(back).reshape(-1), _bits(data))


def test_npy_refusals_write_no_file(app_mod, tmp_path):
    data = np.arange(12, dtype=np.float32)
    path = tmp_path / "no.npy"
    for shape in [(0, 12), (3, 0, 4), (-1, 12), (5, 2), (13,), ()]:
        assert not app_mod.write_npy(path, data, shape), shape
        assert not path.exists()
    assert app_mod.write_npy(path, data, (3, 4))


def test_recorder_files_and_metadata(rec, tmp_path):
    root = tmp_path / "cap"
    rng = np.random.default_rng(5)
    a = rng.random((3, 5, 4), dtype=np.float32)  # height 3, width 5
    b = rng.random((2, 7, 1), dtype=np.float32)
    rec.record_input(a, 5, 3, 4)  # not enabled: ignored, not counted
    assert not root.exists()
    rec.enable(True)
    assert rec.state() == (True, 1, 0, 0)
    rec.record_input(a, 5, 3, 4)  # the default shape
    rec.record_input(b, 7, 2, 1, shape=(2, 7, 1))  # an explicit rank-3 shape is kept as given
    assert rec.state() == (True, 1, 2, 2)
    rec.flush()
    assert _tree(root) == ["inputs/frame_000000.npy", "inputs/frame_000001.npy", "metadata/frame_000000.json",
                           "metadata/frame_000001.json"]
    assert (root / "outputs").is_dir()
    assert (root / "inputs/frame_000000.npy").read_bytes() == tensor_ref.npy_bytes(a, (1, 3, 5, 4))
    assert (root / "metadata/frame_000000.json").read_bytes() == tensor_ref.metadata_text(5, 3, 4, (1, 3, 5, 4)).encode()
    assert b'"colorOrder": "BGRA"' in (root / "metadata/frame_000000.json").read_bytes()
    assert (root / "inputs/frame_000001.npy").read_bytes() == tensor_ref.npy_bytes(b, (2, 7, 1))
    assert (root / "metadata/frame_000001.json").read_bytes() == tensor_ref.metadata_text(7, 2, 1, (2, 7, 1)).encode()
    assert np.array_equal(_bits(np.load(root / "inputs/frame_000000.npy")), _bits(a[None]))


def test_recorder_refusals(rec, tmp_path, capfd):
    root = tmp_path / "cap"
    rec.enable(True)
    good = np.ones((2, 2, 4), np.float32)
    rec.record_output(good, (2, 2, 4))  # no pending input
    assert "no input frame is waiting" in capfd.readouterr().err
    rec.record_input(good, 0, 2, 4)  # a zero dimension
    rec.record_input(good, 2, 2, 0)
    rec.record_input(good, 3, 2, 4)  # a count mismatch
    assert rec.state() == (True, 1, 0, 0)
    assert "rejected a frame" in capfd.readouterr().err
    rec.record_input(good, 2, 2, 4)
    rec.record_output(np.zeros(0, np.float32), (2, 2, 4))  # an empty output: dropped, the input keeps waiting
    assert "empty AI output" in capfd.readouterr().err
    assert rec.state() == (True, 1, 1, 1)
    rec.record_output(good, (2, 0, 4))  # pairs, then the writer refuses the zero dimension: no file
    assert rec.state() == (True, 1, 1, 0)
    rec.record_input(good, 2, 2, 4)
    rec.record_output(good, (1, 2, 2, 5))  # pairs, then the writer refuses the element count
    rec.flush()
    assert _tree(root) == ["inputs/frame_000000.npy", "inputs/frame_000001.npy", "metadata/frame_000000.json",
                           "metadata/frame_000001.json"]


@pytest.mark.parametrize("interval", [1, 3])
def test_interval_and_index_sequence(rec, tmp_path, interval):
    root = tmp_path / "cap"
    rec.set_interval(interval)
    rec.enable(True)
    frames = [np.full((1, 2, 4), k, np.float32) for k in range(7)]
    for f in frames:
        rec.record_input(f, 2, 1, 4)
    kept = [k for k in range(7) if (k + 1) % interval == 0]  # ++counter % interval == 0
    assert rec.state() == (True, interval, len(kept), len(kept))
    rec.enable(False)  # flushes, joins, and resets the numbering and the pending list
    assert rec.state() == (False, interval, 0, 0)
    for i, k in enumerate(kept):
        assert (root / ("inputs/frame_%06d.npy" % i)).read_bytes() == tensor_ref.npy_bytes(frames[k], (1, 1, 2, 4))
    assert len(_tree(root)) == 2 * len(kept)
    # a second session starts at index 0 and at a fresh interval count, whatever the first one left
    rec.record_input(frames[0], 2, 1, 4)  # disabled: not counted
    rec.enable(True)
    for f in frames[4:4 + interval]:
        rec.record_input(f, 2, 1, 4)
    rec.enable(False)
    assert (root / "inputs/frame_000000.npy").read_bytes() == tensor_ref.npy_bytes(frames[4 + interval - 1], (1, 1, 2, 4))
    assert len(_tree(root)) == 2 * len(kept)
    rec.set_interval(0)  # clamped
    assert rec.state()[1] == 1


def test_outputs_pair_with_the_oldest_input(rec, tmp_path):
    root = tmp_path / "cap"
    rec.enable(True)
    ins = [np.full((2, 3, 4), k / 8, np.float32) for k in range(3)]
    for f in ins:
        rec.record_input(f, 3, 2, 4)
    outs = [np.arange(24, dtype=np.float32) + 100 * k for k in range(4)]
    rec.record_output(outs[0], (2, 3, 4))        # rank 3 -> (1, 2, 3, 4), sample 0
    rec.record_output(outs[1], (0, 2, 3, 4))     # batch <= 0 -> 1, sample 1
    rec.record_output(outs[2], None)             # no shape -> (24,) -> (1, 24, 1, 1), sample 2
    rec.record_output(outs[3], (2, 3, 4))        # nothing pending: dropped
    assert rec.state() == (True, 1, 3, 0)
    rec.enable(False)
    want = [(1, 2, 3, 4), (1, 2, 3, 4), (1, 24, 1, 1)]
    for k in range(3):
        assert tuple(tensor_ref.output_shape([(2, 3, 4), (0, 2, 3, 4), ()][k], 24)) == want[k]
        assert (root / ("outputs/ai_%06d.npy" % k)).read_bytes() == tensor_ref.npy_bytes(outs[k], want[k])
    assert not (root / "outputs/ai_000003.npy").exists()
    rec.enable(True)
    rec.record_output(outs[0], (24, 1))  # rank 2 is kept as it is
    rec.record_input(ins[0], 3, 2, 4)
    rec.record_output(outs[3], (24, 1))
    rec.enable(False)
    assert (root / "outputs/ai_000000.npy").read_bytes() == tensor_ref.npy_bytes(outs[3], (24, 1))


def test_empty_directory_falls_back_to_the_working_directory(app_mod, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    r = app_mod.DatasetRecorder()
    r.set_directory("")
    r.enable(True)
    r.record_input(np.zeros((1, 1, 4), np.float32), 1, 1, 4)
    r.close()  # the destructor writes what is queued
    assert (tmp_path / "DatasetCapture/inputs/frame_000000.npy").read_bytes() == tensor_ref.npy_bytes(np.zeros(4), (1, 1, 1, 4))


def _ulp_up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_ai_output_normalisation_is_bit_exact(app_mod, channels):
    rng = np.random.default_rng(channels)
    n = 35 * channels
    unit = rng.random(n, dtype=np.float32)
    unit[:2] = [0.0, 1.0]
    bytes_ = rng.integers(0, 256, n).astype(np.float32)
    hi_edge, lo_edge = np.float32(1) + np.float32(1.0e-3), -np.float32(1.0e-3)
    cases = {
        "unit": unit,
        "bytes": bytes_,
        "at the upper tolerance": np.concatenate([unit[:-1], [hi_edge]]),  # not scaled: clamped to 1
        "one ulp above it": np.concatenate([unit[:-1], [_ulp_up(hi_edge)]]),  # scaled
        "at the lower tolerance": np.concatenate([unit[:-1], [lo_edge]]),  # not scaled: clamped to 0
        "one ulp below it": np.concatenate([unit[:-1], [-_ulp_up(-lo_edge)]]),  # scaled
    }
    scaled = {"bytes", "one ulp above it", "one ulp below it"}
    for name, data in cases.items():
        data = data.astype(np.float32)
        got = app_mod.normalise_ai_output(data, channels)
        want = tensor_ref.normalise_ai_output(data, channels)
        assert np.array_equal(_bits(got), _bits(want)), name
        px = data.reshape(-1, channels)
        first = px[0, 2 if channels >= 3 else 0]  # what lands in channel 0 of pixel 0
        expect0 = np.clip(first * tensor_ref.INV255 if name in scaled else first, 0, 1)
        assert got[0] == np.float32(expect0), name
    # a channel count that does not divide the element count leaves the data alone
    odd = np.arange(7, dtype=np.float32)
    assert np.array_equal(app_mod.normalise_ai_output(odd, 3), odd)


def test_submit_ai_output_checks_the_rank(app_mod):
    a = app_mod.TridentApp()
    data = np.linspace(0, 255, 2 * 3 * 4, dtype=np.float32)
    assert not a.submit_ai_output(data, (24,))
    assert not a.submit_ai_output(data, (6, 4))
    assert not a.submit_ai_output(data, (1, 1, 2, 3, 4))
    assert not a.submit_ai_output(data, ())
    assert a.submit_ai_output(data, (2, 3, 4))
    assert a.submit_ai_output(data, (1, 2, 3, 4))
    assert a.submit_ai_output(data, (-1, 2, 3, 4))  # a dynamic batch
    assert not a.submit_ai_output(data, (1, 2, 3, 3))  # 18 elements described, 24 given
    assert not a.submit_ai_output(np.zeros(0, np.float32), (2, 3, 4))
    a.close()


def test_shim_setters_and_getters(app_mod, tmp_path, monkeypatch):
    monkeypatch.delenv("TRIDENT_DATASET_CAPTURE_ENABLE", raising=False)
    monkeypatch.delenv("TRIDENT_DATASET_CAPTURE_DIR", raising=False)
    monkeypatch.chdir(tmp_path)
    a = app_mod.TridentApp()
    assert a.dataset_capture_state() == (False, str(tmp_path / "DatasetCapture"), 1)
    assert a.ai_readback_enabled() is False
    assert a.acquire_frame() is None and a.readback_device_tensor() is None
    a.set_dataset_capture(True, tmp_path / "d", 5)
    assert a.dataset_capture_state() == (True, str(tmp_path / "d"), 5)
    a.set_dataset_capture(True, None, 0)  # neither changes
    assert a.dataset_capture_state() == (True, str(tmp_path / "d"), 5)
    a.set_dataset_capture(False, "", 0)  # an empty directory: the default
    assert a.dataset_capture_state() == (False, str(tmp_path / "DatasetCapture"), 5)
    assert a.set_ai_readback(True, 0, 0) and a.ai_readback_enabled()
    assert a.set_ai_readback(False) and not a.ai_readback_enabled()
    a.close()
    assert not (tmp_path / "d").exists() and not (tmp_path / "DatasetCapture").exists()  # nothing was recorded


def test_environment_enables_capture_at_init(app_mod, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("TRIDENT_DATASET_CAPTURE_ENABLE", "1")
    monkeypatch.setenv("TRIDENT_DATASET_CAPTURE_DIR", str(tmp_path / "env"))
    a = app_mod.TridentApp()
    assert a.dataset_capture_state() == (True, str(tmp_path / "env"), 1)
    a.close()
    monkeypatch.delenv("TRIDENT_DATASET_CAPTURE_DIR")
    b = app_mod.TridentApp()
    assert b.dataset_capture_state() == (True, str(tmp_path / "DatasetCapture"), 1)
    b.close()
    monkeypatch.setenv("TRIDENT_DATASET_CAPTURE_ENABLE", "")  # empty: not enabled, and the directory is not read
    monkeypatch.setenv("TRIDENT_DATASET_CAPTURE_DIR", str(tmp_path / "env"))
    c = app_mod.TridentApp()
    assert c.dataset_capture_state() == (False, str(tmp_path / "DatasetCapture"), 1)
    c.close()
