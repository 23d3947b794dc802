"""JPEG recording on the GPU: k_jpeg_blocks / k_jpeg_entropy / k_jpeg_offsets / k_jpeg_gather through
tri_recorder_capture_image against the numpy restatement (tests/jpeg_ref.py) with zero differing bytes, the capture
behind a rendered frame, and the slot protocol of a JPEG recorder."""
import io

import numpy as np
import pytest

import jpeg_ref
import scene_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# name: (image, quality, restart_mcus, pitch in pixels or None, what the reference stream must contain)
CASES = {
    "one_mcu": (lambda: jpeg_ref.gradient(16, 16), 90, 0, None, None),
    "padding_both_axes": (lambda: jpeg_ref.gradient(17, 9), 90, 0, None, None),
    "pitched_50x34": (lambda: jpeg_ref.gradient(50, 34), 90, 0, 61, None),
    "restart_1": (lambda: jpeg_ref.gradient(48, 32), 90, 1, None, lambda s: s["intervals"] == 6),
    "restart_3_partial_last": (lambda: jpeg_ref.gradient(48, 32), 90, 3, None, lambda s: s["intervals"] == 2),
    "restart_65535_no_rst": (lambda: jpeg_ref.gradient(48, 32), 90, 65535, None, lambda s: s["intervals"] == 1),
    "nine_intervals_rst0_to_rst7": (lambda: jpeg_ref.noise(32, 144), 50, 2, None,
                                    lambda s: s["intervals"] == 9 and s["rst_markers"] == list(range(0xD0, 0xD8))),
    # 32 x 144 stops one interval short of the wrap (18 MCUs, 8 markers): 32 x 176 has 10, RST7 followed by RST0, RST1
    "rst_wraps": (lambda: jpeg_ref.noise(32, 176), 50, 2, None,
                  lambda s: s["rst_markers"] == list(range(0xD0, 0xD8)) + [0xD0, 0xD1]),
    "intervals_not_dividing_the_row": (lambda: jpeg_ref.gradient(80, 16), 90, 3, None, lambda s: s["intervals"] == 2),
    "intervals_across_rows": (lambda: jpeg_ref.gradient(80, 32), 90, 3, None, lambda s: s["intervals"] == 4),
    "more_intervals_than_waves": (lambda: jpeg_ref.gradient(272, 16), 90, 1, None, lambda s: s["intervals"] == 17),
    "two_scan_chunks": (lambda: jpeg_ref.gradient(272, 256), 90, 1, None, lambda s: s["intervals"] == 272),
    "three_batches_one_interval": (lambda: jpeg_ref.noise(128, 48), 100, 65535, None,
                                   lambda s: s["blocks"] == 144 and s["intervals"] == 1 and s["stuffed"] > 0),
    "two_batches_default_restart": (lambda: jpeg_ref.gradient(400, 16), 90, 0, None, lambda s: s["intervals"] == 3),
    "noise_q100": (lambda: jpeg_ref.noise(48, 32), 100, 0, None,
                   lambda s: s["stuffed"] > 0 and s["blocks_without_eob"] > 0),
    "checker_category_11": (lambda: jpeg_ref.checker(48, 32), 100, 0, None, lambda s: 11 in s["dc_categories"]),
    "zrl": (lambda: jpeg_ref.high_frequency(32, 16), 90, 0, None, lambda s: s["ac_symbols"].get(0xF0, 0) > 0),
    "black": (lambda: jpeg_ref.black(32, 32), 90, 0, None, lambda s: s["dc_only_blocks"] == s["blocks"]),
    "quality_1": (lambda: jpeg_ref.gradient(50, 34), 1, 0, None, None),
    "quality_100": (lambda: jpeg_ref.gradient(50, 34), 100, 0, None, None),
}
_REFERENCE = {}


def reference(name):
    if name not in _REFERENCE:
        make, quality, restart, _, must = CASES[name]
        image, stats = make(), {}
        stream = jpeg_ref.encode(image, quality, restart, stats=stats)
        if must is not None:
            assert must(stats), (name, {k: v for k, v in stats.items() if k != "ac_symbols"})
        _REFERENCE[name] = (image, stream)
    return _REFERENCE[name]


def _device_image(image, pitch_pixels):
    import torch

    h, w = image.shape[:2]
    if pitch_pixels is None:
        t = torch.from_numpy(image).to(DEV)
        return t, t, w * 4
    whole = np.random.default_rng(5).integers(0, 256, (h + 1, pitch_pixels, 4), dtype=np.uint8)
    whole[1:, 4:4 + w] = image  # (the window starts one row and 16 bytes into the wider image)
    t = torch.from_numpy(whole).to(DEV)
    return t, t[1:, 4:], pitch_pixels * 4


@pytest.mark.parametrize("name", list(CASES))
def test_device_stream_equals_the_restatement(name):
    import torch
    from trident_raster import abi, raster

    image, want = reference(name)
    _, quality, restart, pitch_pixels, _ = CASES[name]
    h, w = image.shape[:2]
    keep, window, pitch = _device_image(image, pitch_pixels)
    torch.cuda.synchronize()
    with raster.TriRecorder(w, h, 1, fmt=abi.TRI_RECORD_JPEG420, quality=quality, restart_mcus=restart) as rec:
        rec.capture_image(0, window.data_ptr(), pitch)
        got = bytes(rec.wait_ex(0))
        rec.release(0)
    assert len(got) == len(want)
    assert sum(a != b for a, b in zip(got, want)) == 0
    assert len(got) <= raster.jpeg_max_bytes(w, h, quality, restart)
    del keep


def test_pillow_decodes_the_device_stream():
    """12 MCUs at one per interval: 11 markers, so the decoder follows RST7 with RST0, RST1, RST2."""
    import torch
    from PIL import Image
    from trident_raster import abi, raster

    image = jpeg_ref.gradient(50, 34)
    t = torch.from_numpy(image).to(DEV)
    torch.cuda.synchronize()
    with raster.TriRecorder(50, 34, 1, fmt=abi.TRI_RECORD_JPEG420, quality=95, restart_mcus=1) as rec:
        rec.capture_image(0, t.data_ptr(), 200)
        got = bytes(rec.wait_ex(0))
    assert got.count(b"\xFF\xD0") >= 2 and got.count(b"\xFF\xD7") >= 1
    im = Image.open(io.BytesIO(got))
    im.load()
    assert im.size == (50, 34)
    err = np.asarray(im.convert("RGB")).astype(int) - image[..., [2, 1, 0]].astype(int)
    assert 10 * np.log10(255.0 ** 2 / (err ** 2).mean()) > 25.0


def test_capture_behind_rendered_frames_on_three_contexts():
    """tri_recorder_capture behind tri_render, three slots in flight on three contexts before any is collected: each
    equals the restatement of that context's tri_readback pixels, and the frames are the ones the contexts render
    without a recorder."""
    from trident_raster import abi, raster, scenes

    frames = [sc.c1_cube_skybox(f, 100, 70) for f in (0, 1, 2)]
    plain = []
    for s in frames:
        with raster.TriRaster(100, 70) as ref:
            scenes.load_scene(ref, s)
            ref.render_frame()
            plain.append(ref.readback())
    assert not np.array_equal(plain[0][0], plain[1][0]) and not np.array_equal(plain[1][0], plain[2][0])
    assert len(np.unique(plain[1][0].reshape(-1, 4), axis=0)) > 50  # a picture, not a flat frame
    ctxs = [raster.TriRaster(100, 70) for _ in frames]
    try:
        with raster.TriRecorder(100, 70, 3, fmt=abi.TRI_RECORD_JPEG420) as rec:
            for k, (r, s) in enumerate(zip(ctxs, frames)):
                scenes.load_scene(r, s)
                r.render()
                rec.capture(2 - k, r)
            got = [bytes(rec.wait_ex(2 - k)) for k in range(3)]
            for k in range(3):
                rec.release(k)
        for k, r in enumerate(ctxs):
            col, dep = r.readback()
            assert np.array_equal(col, plain[k][0]) and np.array_equal(dep, plain[k][1])
            assert got[k] == jpeg_ref.encode(col)
    finally:
        for r in ctxs:
            r.close()


def test_three_slots_in_flight_and_the_slot_protocol(hiplib):
    import ctypes as C

    import torch
    from trident_raster import abi, raster

    def fails(code, fn, *args):
        with pytest.raises(raster.TriError) as ei:
            fn(*args)
        assert ei.value.code == code
        assert hiplib.tri_last_error()

    images = [jpeg_ref.gradient(50, 34, seed=k) for k in range(3)]
    want = [jpeg_ref.encode(i, 80, 2) for i in images]
    assert len(set(want)) == 3
    tensors = [torch.from_numpy(i).to(DEV) for i in images]
    streams = [torch.cuda.Stream() for _ in range(3)]
    torch.cuda.synchronize()
    with raster.TriRecorder(50, 34, 3, fmt=abi.TRI_RECORD_JPEG420, quality=80, restart_mcus=2) as rec:
        fails(abi.TRI_E_STATE, rec.wait_ex, 0)  # idle
        for k in range(3):
            rec.capture_image(k, tensors[k].data_ptr(), 200, streams[k].cuda_stream)
        fails(abi.TRI_E_STATE, rec.capture_image, 0, tensors[0].data_ptr(), 200)  # busy
        fails(abi.TRI_E_STATE, rec.wait_pointer, 0)  # tri_recorder_wait has no size to give
        fails(abi.TRI_E_INVALID, rec.capture_image, 3, tensors[0].data_ptr(), 200)
        fails(abi.TRI_E_INVALID, rec.wait_ex, 3)
        fails(abi.TRI_E_INVALID, rec.capture_image, 1, None, 200)
        fails(abi.TRI_E_INVALID, rec.capture_image, 1, tensors[0].data_ptr(), 196)  # below 4 * width
        fails(abi.TRI_E_INVALID, rec.capture_image, 1, tensors[0].data_ptr(), 202)  # not a multiple of 4
        for k in (2, 0, 1):
            assert bytes(rec.wait_ex(k)) == want[k]
        assert bytes(rec.wait_ex(0)) == want[0]  # any number of waits
        rec.release(0)
        fails(abi.TRI_E_STATE, rec.wait_ex, 0)
        rec.capture_image(0, tensors[2].data_ptr(), 200)  # a released slot serves again
        assert bytes(rec.wait_ex(0)) == want[2]
        with raster.TriRaster(64, 34) as other:
            fails(abi.TRI_E_INVALID, rec.capture, 1, other)  # busy or not, another extent is refused first
        rec.release(1)
        with raster.TriRaster(64, 34) as other:
            fails(abi.TRI_E_INVALID, rec.capture, 1, other)
        with raster.TriRaster(50, 34, band=(0, 16)) as band:
            fails(abi.TRI_E_STATE, rec.capture, 1, band)
    # destroyed with a capture in flight that nobody waited for
    rec = raster.TriRecorder(50, 34, 2, fmt=abi.TRI_RECORD_JPEG420)
    rec.capture_image(1, tensors[1].data_ptr(), 200, streams[1].cuda_stream)
    rec.close()
    torch.cuda.synchronize()
    # the create's own refusals need no capture
    for bad in (dict(quality=0), dict(quality=101), dict(restart_mcus=65536), dict(fmt=2)):
        fails(abi.TRI_E_INVALID, lambda kw: raster.TriRecorder(50, 34, 1, **{"fmt": abi.TRI_RECORD_JPEG420, **kw}), bad)
    p = abi.TriRecordParams(abi.TRI_RECORD_JPEG420, 90, 0, 1)
    fails(abi.TRI_E_INVALID, lambda: raster.TriRecorder(50, 34, 1, params=p))
    out = C.c_void_p(1)
    assert hiplib.tri_recorder_create_ex(-1, 50, 34, 9, None, C.byref(out)) == abi.TRI_E_INVALID and not out.value


def test_yuv444_through_create_ex_is_the_plain_recorder():
    import torch
    from trident_raster import abi, raster

    image = jpeg_ref.noise(50, 34)
    t = torch.from_numpy(image).to(DEV)
    torch.cuda.synchronize()
    with raster.TriRecorder(50, 34, 1) as plain, raster.TriRecorder(50, 34, 1, fmt=abi.TRI_RECORD_YUV444) as ex:
        plain.capture_image(0, t.data_ptr(), 200)
        ex.capture_image(0, t.data_ptr(), 200)
        a = plain.wait(0).copy()
        b = ex.wait_ex(0)
        assert b.size == 3 * 50 * 34
        assert np.array_equal(a.reshape(-1), b)
        assert np.array_equal(ex.wait(0), a)  # tri_recorder_wait still serves a YUV444 recorder
