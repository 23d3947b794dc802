"""tri_nn_conv on the GPU, one layer at a time, bit for bit against torch.nn.functional on the CPU.

The data are exact integers: inputs and residuals in [-4, 4], weights in [-3, 3] drawn independently per
(tap, ci, co) — a swapped tap, a transposed channel pair or a flipped kernel changes the result — scales in
{0.5, 1, 2} and integer shifts. With K = taps x Cin <= 1152 every partial sum is below 2^24 in magnitude
(1152 * 4 * 3 = 13824), so the float32 result does not depend on the summation order and must be exact. Guard bytes
around every output must be untouched. (The sigmoid is checked through the end-to-end test, test_framegen_gpu.)"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from trident_raster import abi

pytestmark = pytest.mark.gpu

GUARD = 1024  # bytes on each side of an output
# one row and one column beyond the largest spatial tile of the stride-1 and transposed kernels (16 x 32; the
# 64-channel-wide variant's is 8 x 32)
PAST_TILE = (17, 33)


def _case_data(op, cin, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (h, w, cin), generator=g).to(torch.float32)
    wshape = (cout, cin, 3, 3) if op == abi.TRI_NN_CONV3X3 else (cin, cout, 4, 4)
    wt = torch.randint(-3, 4, wshape, generator=g).to(torch.float32)
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (cout,), generator=g)]
    shift = torch.randint(-5, 6, (cout,), generator=g).to(torch.float32)
    return x, wt, scale, shift, g


def _run(hiplib, op, stride, x, wt, scale, shift, act, res1, res2, out_hw):
    h, w, cin = x.shape
    cout = scale.numel()
    desc = abi.TriNnConvDesc(op, stride, h, w, cin, cout, act, 0)
    src = np.ascontiguousarray(wt.numpy())
    packed = np.empty(src.size, np.float32)
    assert hiplib.tri_nn_pack_weights(C.byref(desc), src.ctypes.data, packed.ctypes.data) == abi.TRI_OK
    dev = lambda t: None if t is None else t.contiguous().cuda()  # noqa: E731
    dx, dw, ds, db, d1, d2 = dev(x), dev(torch.from_numpy(packed)), dev(scale), dev(shift), dev(res1), dev(res2)
    n = out_hw[0] * out_hw[1] * cout * 4
    whole = torch.full((GUARD + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out_ptr = whole.data_ptr() + GUARD
    assert out_ptr % 4 == 0
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    rc = hiplib.tri_nn_conv(C.byref(desc), ptr(dx), ptr(dw), ptr(ds), ptr(db), ptr(d1), ptr(d2), C.c_void_p(out_ptr), None)
    assert rc == abi.TRI_OK, hiplib.tri_last_error()
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + n:] == 0xA5), "guard bytes were written"
    return got[GUARD:GUARD + n].view(np.float32).reshape(out_hw[0], out_hw[1], cout)


def _reference(op, stride, x, wt, scale, shift, act, res1, res2):
    xc = x.permute(2, 0, 1)[None]
    if op == abi.TRI_NN_CONV3X3:
        y = F.conv2d(xc, wt, None, stride=stride, padding=1)
    else:
        y = F.conv_transpose2d(xc, wt, None, stride=2, padding=1)
    y = y[0].permute(1, 2, 0) * scale + shift
    if res1 is not None:
        y = y + res1
    if act == abi.TRI_NN_ACT_RELU:
        y = F.relu(y)
    if res2 is not None:
        y = y + res2
    return y.contiguous().numpy()


EPILOGUES = ["none", "relu", "res1", "res2"]


def _check(hiplib, op, stride, cin, cout, h, w, epilogue, seed):
    x, wt, scale, shift, g = _case_data(op, cin, cout, h, w, seed)
    oh, ow = (2 * h, 2 * w) if op == abi.TRI_NN_CONVT4X4 else ((h + stride - 1) // stride, (w + stride - 1) // stride)
    res = lambda: torch.randint(-4, 5, (oh, ow, cout), generator=g).to(torch.float32)  # noqa: E731
    # "res1" is a residual block's last layer (added before the ReLU), "res2" a decoder stage's (both, the skip after it)
    res1 = res() if epilogue in ("res1", "res2") else None
    res2 = res() if epilogue == "res2" else None
    act = abi.TRI_NN_ACT_NONE if epilogue == "none" else abi.TRI_NN_ACT_RELU
    want = _reference(op, stride, x, wt, scale, shift, act, res1, res2)
    assert want.shape == (oh, ow, cout) and np.abs(want).max() < 2 ** 24
    got = _run(hiplib, op, stride, x, wt, scale, shift, act, res1, res2, (oh, ow))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{int((got != want).sum())} of {want.size} differ, max {np.abs(got - want).max()}"


@pytest.mark.parametrize("epilogue", EPILOGUES)
@pytest.mark.parametrize("channels", [(4, 32), (6, 32), (32, 32), (128, 128), (32, 3)])
@pytest.mark.parametrize("size", [(1, 1), (5, 7), PAST_TILE])
def test_conv3x3_stride1_exact(hiplib, size, channels, epilogue):
    _check(hiplib, abi.TRI_NN_CONV3X3, 1, channels[0], channels[1], size[0], size[1], epilogue, seed=11)


@pytest.mark.parametrize("channels", [(32, 64), (64, 128)])
@pytest.mark.parametrize("size", [(5, 7), (8, 12), (35, 33)])  # odd: the output is ceil(H / 2); 35 x 33: past the 16 x 16 tile
def test_conv3x3_stride2_exact(hiplib, size, channels):
    _check(hiplib, abi.TRI_NN_CONV3X3, 2, channels[0], channels[1], size[0], size[1], "relu", seed=12)


@pytest.mark.parametrize("channels", [(128, 64), (64, 32)])
@pytest.mark.parametrize("size", [(1, 1), (3, 5), PAST_TILE])
def test_conv_transpose4x4_exact(hiplib, size, channels):
    _check(hiplib, abi.TRI_NN_CONVT4X4, 2, channels[0], channels[1], size[0], size[1], "relu", seed=13)


def test_bad_descriptors_are_refused(hiplib):
    p = C.c_void_p(256)
    for bad in [abi.TriNnConvDesc(2, 1, 4, 4, 4, 4, 0, 0), abi.TriNnConvDesc(0, 3, 4, 4, 4, 4, 0, 0),
                abi.TriNnConvDesc(1, 1, 4, 4, 4, 4, 0, 0), abi.TriNnConvDesc(0, 1, 0, 4, 4, 4, 0, 0),
                abi.TriNnConvDesc(0, 1, 4, 4, 0, 4, 0, 0), abi.TriNnConvDesc(0, 1, 4, 4, 4, 2000, 0, 0),
                abi.TriNnConvDesc(0, 1, 4, 4, 4, 4, 3, 0), abi.TriNnConvDesc(1, 2, 5000, 4, 4, 4, 0, 0)]:
        assert hiplib.tri_nn_conv(C.byref(bad), p, p, p, p, None, None, C.c_void_p(512), None) == abi.TRI_E_INVALID
        assert b"tri_nn_conv" in hiplib.tri_last_error()
    ok = abi.TriNnConvDesc(0, 1, 4, 4, 4, 4, 0, 0)
    assert hiplib.tri_nn_conv(C.byref(ok), p, p, p, p, None, None, None, None) == abi.TRI_E_INVALID
    assert hiplib.tri_nn_conv(C.byref(ok), C.c_void_p(258), p, p, p, None, None, C.c_void_p(512), None) == abi.TRI_E_INVALID
