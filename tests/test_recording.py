"""Viewport recording, the host side (no GPU): the restated conversion itself, the shim's converter against it on
every RGB triple, and Trident::VideoEncoder's Y4M sessions (header, FRAME records, the session rules of
VideoEncoder.cpp:19-85, :187-225, :370-412)."""
import ctypes as C
import os

import numpy as np
import pytest

import yuv_ref


@pytest.fixture(scope="module")
def app_mod():
    from trident_raster import app

    app.load_library()
    return app


@pytest.fixture()
def enc(app_mod):
    e = app_mod.VideoEncoder()
    yield e
    e.close()


def test_restatement_pins():
    """Guards the yardstick: the truncated double sums, and how often they differ from the exact integer floor."""
    grey = lambda v: tuple(int(x) for x in yuv_ref.yuv444(np.array([v, v, v], np.uint8)))  # noqa: E731
    assert grey(128) == (127, 128, 128)  # 0.299 * 128 + 0.587 * 128 + 0.114 * 128 < 128 in double
    assert grey(1) == (0, 128, 128)
    assert grey(255) == (255, 128, 128)
    rgb, yuv = yuv_ref.all_triples()
    r, g, b = (rgb[:, k].astype(np.int64) for k in range(3))
    floor_y = (299 * r + 587 * g + 114 * b) // 1000
    floor_u = (-169 * r - 331 * g + 500 * b + 128000) // 1000
    floor_v = (500 * r - 419 * g - 81 * b + 128000) // 1000
    assert int((yuv[0] != floor_y).sum()) == 3464
    assert int((yuv[1] != floor_u).sum()) == 1393
    assert int((yuv[2] != floor_v).sum()) == 0


def test_host_converter_matches_on_every_triple(app_mod):
    rgb, want = yuv_ref.all_triples()
    rgba = np.empty((1 << 24, 4), np.uint8)
    rgba[:, :3] = rgb
    rgba[:, 3] = rgb[:, 0] ^ rgb[:, 1] ^ rgb[:, 2]  # alpha varies and is ignored
    got = app_mod.convert_rgba(rgba)
    for k, name in enumerate("YUV"):
        assert int((got[k] != want[k]).sum()) == 0, name


def _records(data, width, height, fps):
    """Splits a Y4M file into its FRAME payloads after checking the header and every record marker."""
    head = yuv_ref.y4m_header(width, height, fps)
    assert data[:len(head)] == head
    body, size = data[len(head):], 6 + 3 * width * height
    assert len(body) % size == 0
    recs = [body[i:i + size] for i in range(0, len(body), size)]
    assert all(r[:6] == b"FRAME\n" for r in recs)
    return [np.frombuffer(r[6:], np.uint8).reshape(3, height, width) for r in recs]


def test_encoder_writes_a_valid_file(enc, tmp_path):
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (5, 7, 4), dtype=np.uint8) for _ in range(3)]  # 7 x 5: odd, not rounded here
    path = tmp_path / "odd.y4m"
    assert enc.begin(path, 7, 5, 24)
    assert enc.state() == (True, 0)
    for f in frames:
        assert enc.submit_rgba(f, 7, 5)
    assert enc.state() == (True, 3)
    assert enc.end()
    assert enc.state() == (False, 3)
    data = path.read_bytes()
    assert data.startswith(b"YUV4MPEG2 W7 H5 F24:1 Ip A0:0 C444\n")
    recs = _records(data, 7, 5, 24)
    assert len(recs) == 3
    for got, f in zip(recs, frames):
        assert np.array_equal(got, yuv_ref.yuv444(f))
    assert data == yuv_ref.y4m_file(7, 5, 24, frames)


def test_encoder_extension_case_and_default_fps(enc, tmp_path):
    path = tmp_path / "UPPER.Y4M"
    assert enc.begin(path, 2, 2, 0)  # fps 0 means 30
    assert enc.end()
    assert path.read_bytes() == b"YUV4MPEG2 W2 H2 F30:1 Ip A0:0 C444\n"


def test_planes_and_frames_write_the_same_bytes(app_mod, tmp_path):
    rng = np.random.default_rng(11)
    f = rng.integers(0, 256, (6, 9, 4), dtype=np.uint8)
    a, b = app_mod.VideoEncoder(), app_mod.VideoEncoder()
    assert a.begin(tmp_path / "a.y4m", 9, 6, 1) and b.begin(tmp_path / "b.y4m", 9, 6, 1)
    assert a.submit_rgba(f, 9, 6)
    assert b.submit_planes(yuv_ref.yuv444(f), 9, 6)
    assert a.end() and b.end()
    assert (tmp_path / "a.y4m").read_bytes() == (tmp_path / "b.y4m").read_bytes() == yuv_ref.y4m_file(9, 6, 1, [f])


@pytest.mark.parametrize("name,width,height", [("a.mp4", 4, 4), ("a.mov", 4, 4), ("a.avi", 4, 4), ("a.MP4", 4, 4),
                                               ("a.bin", 4, 4), ("y4m", 4, 4), ("a.y4m", 0, 4), ("a.y4m", 4, 0)])
def test_encoder_refuses_and_creates_no_file(enc, tmp_path, capfd, name, width, height):
    path = tmp_path / name
    assert not enc.begin(path, width, height, 30)
    assert enc.state() == (False, 0)
    assert not path.exists()
    assert os.listdir(tmp_path) == []
    if name.lower().endswith((".mp4", ".mov", ".avi")):
        assert "FFmpeg" in capfd.readouterr().err  # the documented deviation says why


def test_encoder_refuses_bad_frames(enc, tmp_path):
    f = np.full((4, 6, 4), 200, np.uint8)
    assert not enc.submit_rgba(f, 6, 4)  # before any session
    assert not enc.submit_planes(yuv_ref.yuv444(f), 6, 4)
    assert not enc.end()
    path = tmp_path / "s.y4m"
    assert enc.begin(path, 6, 4, 5)
    assert enc.submit_rgba(f, 6, 4)
    assert not enc.submit_rgba(np.zeros((6, 4, 4), np.uint8), 4, 6)  # another extent
    assert not enc.submit_planes(np.zeros(3 * 4 * 6, np.uint8), 4, 6)
    assert not enc.submit_rgba(np.zeros(0, np.uint8), 6, 4)  # an empty pixel buffer
    assert enc.state() == (True, 1)
    assert enc.end()
    assert not enc.end()  # the session is over
    assert not enc.submit_rgba(f, 6, 4)
    assert path.read_bytes() == yuv_ref.y4m_file(6, 4, 5, [f])  # the refused frames added no bytes


def test_begin_ends_the_running_session(enc, tmp_path):
    f = np.full((2, 2, 4), 9, np.uint8)
    assert enc.begin(tmp_path / "one.y4m", 2, 2, 1) and enc.submit_rgba(f, 2, 2)
    assert enc.begin(tmp_path / "two.y4m", 2, 2, 1)
    assert enc.state() == (True, 0)
    assert enc.end()
    assert (tmp_path / "one.y4m").read_bytes() == yuv_ref.y4m_file(2, 2, 1, [f])
    assert (tmp_path / "two.y4m").read_bytes() == yuv_ref.y4m_header(2, 2, 1)


def test_recording_entry_points_are_declared_and_check_arguments(hiplib):
    """The C-ABI additions are mirrored (tests/test_abi.py compares the whole list) and reject bad arguments before
    touching a device; the version stays 2."""
    from trident_raster import abi

    names = {n for n, _, _ in abi.CABI_FUNCTIONS}
    assert {"tri_convert_yuv444", "tri_recorder_create", "tri_recorder_destroy", "tri_recorder_capture",
            "tri_recorder_wait", "tri_recorder_release"} <= names
    assert hiplib.tri_abi_version() == 2
    fake = C.c_void_p(0x1000)  # never dereferenced: every call below fails its argument check
    assert hiplib.tri_convert_yuv444(None, 4, 4, 16, fake, None) == abi.TRI_E_INVALID
    assert hiplib.tri_convert_yuv444(fake, 4, 4, 16, None, None) == abi.TRI_E_INVALID
    assert hiplib.tri_convert_yuv444(fake, 0, 4, 16, fake, None) == abi.TRI_E_INVALID
    assert hiplib.tri_convert_yuv444(fake, 4, 8193, 16, fake, None) == abi.TRI_E_INVALID
    assert hiplib.tri_convert_yuv444(fake, 4, 4, 12, fake, None) == abi.TRI_E_INVALID
    assert hiplib.tri_convert_yuv444(fake, 4, 4, 18, fake, None) == abi.TRI_E_INVALID
    assert hiplib.tri_convert_yuv444(C.c_void_p(0x1002), 4, 4, 16, fake, None) == abi.TRI_E_INVALID
    assert hiplib.tri_last_error()
    out = C.c_void_p()
    assert hiplib.tri_recorder_create(-1, 4, 4, 0, C.byref(out)) == abi.TRI_E_INVALID
    assert hiplib.tri_recorder_create(-1, 4, 4, 9, C.byref(out)) == abi.TRI_E_INVALID
    assert hiplib.tri_recorder_create(-1, 0, 4, 2, C.byref(out)) == abi.TRI_E_INVALID
    assert not out.value
    assert hiplib.tri_recorder_destroy(None) == abi.TRI_OK
    assert hiplib.tri_recorder_capture(None, 0, None) == abi.TRI_E_INVALID
