"""The frame generator end to end on the GPU: a seeded network in a weights container, 20 layers on the device, against
the network restated in torch on the CPU (framegen_ref).

The reference is the float64 run R64. The float32 run R32 of the same restatement gives the reference's own rounding
noise e_ref = max|R32 - R64|; the device result is another float32 summation order of the same products, so it must
stay within BOUND_M * e_ref. BOUND_M (framegen_ref) is the largest ratio max|GPU - R64| / e_ref measured on the MI355X
over the three shapes (DESIGN 5k lists them), rounded up to a power of two; it may never exceed 16 — a larger ratio is
a defect."""
import ctypes as C

import numpy as np
import pytest
import torch

import framegen_ref
from trident_raster import abi, raster

pytestmark = pytest.mark.gpu

BOUND_M = framegen_ref.BOUND_M

# (height, width, input channels): the bottleneck is 1 x 1; 2 x 3; 5 x 9 (odd on both sides)
SHAPES = [(4, 4, 4), (8, 12, 4), (20, 36, 6)]


class Case:
    def __init__(self, h, w, cin):
        seed = 1000 + h * w + cin
        self.h, self.w, self.cin = h, w, cin
        self.state = framegen_ref.make_state(cin, seed)
        self.x = torch.rand((h, w, cin), generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float32).numpy()
        self.r64 = framegen_ref.forward(self.state, self.x, torch.float64)
        self.r32 = framegen_ref.forward(self.state, self.x, torch.float32)
        self.e_ref = float(np.abs(self.r32.astype(np.float64) - self.r64).max())
        self.container = framegen_ref.container_bytes(self.state, cin)
        self._gpu = None

    def gpu(self):
        """(output float32 [h, w, 3], packed blend frame uint8 [h, w, 4]) of one run on the device."""
        if self._gpu is None:
            x = torch.from_numpy(self.x).cuda()
            with raster.FrameGenerator(self.container, self.w, self.h) as gen, raster.TriRaster(self.w, self.h) as ctx:
                assert gen.input_channels == self.cin
                gen.submit(x.data_ptr())
                gen.wait()
                out = gen.read_output()
                assert gen.last_ms() > 0.0
                ctx.upload_ai_frame_device(gen.output_pointer(), self.w, self.h, 3, behind=gen)
                packed = ctx.read_ai_frame(self.w, self.h)
            self._gpu = (out, packed)
        return self._gpu


@pytest.fixture(scope="module")
def cases():
    return {s: Case(*s) for s in SHAPES}


@pytest.mark.parametrize("shape", SHAPES)
def test_device_network_within_the_reference_noise(cases, shape):
    c = cases[shape]
    out, _ = c.gpu()
    err = float(np.abs(out.astype(np.float64) - c.r64).max())
    print(f"framegen {shape}: e_ref {c.e_ref:.3e} gpu error {err:.3e} ratio {err / c.e_ref:.3f} "
          f"output range [{out.min():.3f}, {out.max():.3f}]")
    assert c.e_ref > 0.0 and out.max() - out.min() > 0.2  # a flat output would check nothing
    assert err <= BOUND_M * c.e_ref, (err, c.e_ref, err / c.e_ref)


@pytest.mark.parametrize("shape", SHAPES)
def test_bound_rejects_a_mirrored_kernel(cases, shape):
    """On the CPU: the same network with one 3x3 kernel mirrored misses even the 16 * e_ref ceiling by far, and one
    transposed convolution flipped more so — the bound tells defects from rounding."""
    c = cases[shape]
    mirrored = framegen_ref.forward(c.state, c.x, torch.float32, mirror="m_EncoderStage2.2.m_Block.3")
    flipped = framegen_ref.forward(c.state, c.x, torch.float32, flip_transposed="m_DecodeStage1.0")
    e_mirror = float(np.abs(mirrored.astype(np.float64) - c.r64).max())
    e_flip = float(np.abs(flipped.astype(np.float64) - c.r64).max())
    print(f"framegen {shape}: mirrored {e_mirror:.3e} flipped {e_flip:.3e} e_ref {c.e_ref:.3e}")
    assert e_mirror > 100 * 16 * c.e_ref and e_flip > 100 * 16 * c.e_ref


@pytest.mark.parametrize("shape", SHAPES)
def test_packed_frame_within_one_lsb(cases, shape):
    c = cases[shape]
    _, packed = c.gpu()
    want = framegen_ref.pack_rgba8(c.r32)
    assert np.array_equal(framegen_ref.pack_rgba8(c.r64.astype(np.float32)), want)  # R32 and R64 pack alike
    assert np.array_equal(packed[..., 3], want[..., 3])
    assert np.abs(packed.astype(np.int16) - want.astype(np.int16)).max() <= 1


@pytest.mark.parametrize("channels", [3, 4])
def test_ai_pack_bit_exact(channels):
    """k_ai_pack alone against the host packing restated in numpy float32: every n / 255, its float neighbours, the
    floats around (n + 0.5) / 255 where the rounding flips, and values the clamp catches."""
    n = np.arange(256, dtype=np.float32)
    exact = n / np.float32(255)
    halves = ((n.astype(np.float64) + 0.5) / 255.0).astype(np.float32)
    values = np.concatenate([exact, np.nextafter(exact, np.float32(-1)), np.nextafter(exact, np.float32(2)),
                             halves, np.nextafter(halves, np.float32(-1)), np.nextafter(halves, np.float32(2)),
                             np.array([-0.0, -1.0e-3, -5.0, 1.0 + 1.0e-3, 7.0, 1.0e-30, 0.999999], np.float32)])
    width, height = 64, -(-values.size * 2 // 64 // channels) + 1
    count = width * height * channels
    rng = np.random.default_rng(5)
    tensor = np.concatenate([values, rng.choice(values, count - values.size)]).astype(np.float32).reshape(height, width, channels)
    dev = torch.from_numpy(tensor).cuda()
    with raster.TriRaster(width, height) as ctx:
        ctx.upload_ai_frame_device(dev.data_ptr(), width, height, channels)
        got = ctx.read_ai_frame(width, height)
    want = framegen_ref.pack_rgba8(tensor)
    assert np.array_equal(got, want), int((got != want).sum())


def test_protocol(cases, hiplib):
    c = cases[(8, 12, 4)]
    x = torch.from_numpy(c.x).cuda()
    gen = raster.FrameGenerator(c.container, c.w, c.h)
    assert gen.poll() is False  # before any submit
    with pytest.raises(raster.TriError) as e:
        gen.wait()
    assert e.value.code == abi.TRI_E_STATE
    with pytest.raises(raster.TriError) as e:
        gen.read_output()
    assert e.value.code == abi.TRI_E_STATE
    gen.submit(x.data_ptr())
    with pytest.raises(raster.TriError) as e:  # in flight until a poll or a wait has seen it finish
        gen.submit(x.data_ptr())
    assert e.value.code == abi.TRI_E_STATE
    gen.wait()
    assert gen.poll() is False  # the wait consumed the job
    first = gen.read_output()
    gen.submit(x.data_ptr())
    gen.close()  # destroy with a job in flight waits
    assert np.array_equal(first, c.gpu()[0])  # the same input gives the same bits

    handle = C.c_void_p(1)
    rc = hiplib.tri_framegen_create(-1, c.container, len(c.container), 8, 6, C.byref(handle))
    assert rc == abi.TRI_E_INVALID and not handle.value and b"multiples of 4" in hiplib.tri_last_error()
    assert hiplib.tri_framegen_create(-1, c.container, len(c.container), 8, 8196, C.byref(handle)) == abi.TRI_E_INVALID
    assert hiplib.tri_framegen_destroy(None) == abi.TRI_OK


def test_poll_reports_a_finished_job_once(cases):
    c = cases[(4, 4, 4)]
    x = torch.from_numpy(c.x).cuda()
    with raster.FrameGenerator(c.container, c.w, c.h) as gen:
        gen.submit(x.data_ptr())
        torch.cuda.synchronize()  # every stream of the device: the job has finished
        assert gen.poll() is True
        assert gen.poll() is False
        assert np.array_equal(gen.read_output(), c.gpu()[0])
