"""The frame generator tests' yardstick: the interpolation network restated functionally in torch (any dtype, on the
CPU), seeded weights under the checkpoint's state_dict keys, the weights container, and the host packing of a
generated frame restated in numpy float32.

The network: three encoder stages (a 3x3 convolution with bias and ReLU, then a residual block; stages 2 and 3 at
stride 2), two bottleneck residual blocks, two decoder stages (a 4x4 stride-2 transposed convolution with bias and
ReLU, a residual block, plus the encoder's skip added after the block's ReLU), a final 3x3 convolution and a sigmoid.
A residual block is conv, BatchNorm (eval), ReLU, conv, BatchNorm, plus its input, ReLU; its convolutions have no bias.
"""
import struct

import numpy as np
import torch
import torch.nn.functional as F

ENCODER = [("m_EncoderStage1", None, 32, 1), ("m_EncoderStage2", 32, 64, 2), ("m_EncoderStage3", 64, 128, 2)]
DECODER = [("m_DecodeStage2", 128, 64), ("m_DecodeStage1", 64, 32)]
BLOCKS = [("m_EncoderStage1.2", 32), ("m_EncoderStage2.2", 64), ("m_EncoderStage3.2", 128), ("m_Bottleneck.0", 128),
          ("m_Bottleneck.1", 128), ("m_DecodeStage2.2", 64), ("m_DecodeStage1.2", 32)]
EPS = 1.0e-5
MAGIC, VERSION, HEADER_BYTES, ENTRY_BYTES = b"TRIFGEN\0", 1, 32, 96
# The device network must stay within BOUND_M * e_ref of the float64 reference, e_ref being the float32 reference's own
# distance from it. Measured on the MI355X: max|GPU - R64| / e_ref = 1.27, 1.05, 1.05 on the three shapes of
# test_framegen_gpu; the largest, rounded up to a power of two. It may never exceed 16: a larger ratio is a defect.
BOUND_M = 2
assert BOUND_M <= 16


def make_state(input_channels, seed):
    """A float32 state_dict: torch's default convolution ranges (U(-1/sqrt(fan_in), 1/sqrt(fan_in)) for weight and
    bias), BatchNorm gamma and variance in U(0.5, 1.5), beta and mean ~ N(0, 0.1), and the final layer scaled by 8 so the
    sigmoid's output is not flat."""
    g = torch.Generator().manual_seed(seed)
    state = {}

    def uniform(shape, bound):
        return (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound

    def conv(prefix, cout, cin, k, bias, transposed=False, gain=1.0):
        shape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
        fan_in = shape[1] * k * k  # torch counts dim 1 for both
        bound = 1.0 / fan_in ** 0.5
        state[prefix + ".weight"] = uniform(shape, bound) * gain
        if bias:
            state[prefix + ".bias"] = uniform((cout,), bound) * gain

    def norm(prefix, c):
        state[prefix + ".weight"] = torch.rand(c, generator=g) + 0.5
        state[prefix + ".bias"] = torch.randn(c, generator=g) * 0.1
        state[prefix + ".running_mean"] = torch.randn(c, generator=g) * 0.1
        state[prefix + ".running_var"] = torch.rand(c, generator=g) + 0.5
        state[prefix + ".num_batches_tracked"] = torch.tensor(7, dtype=torch.int64)

    for name, cin, cout, _ in ENCODER:
        conv(name + ".0", cout, cin or input_channels, 3, True)
    for name, cin, cout in DECODER:
        conv(name + ".0", cout, cin, 4, True, transposed=True)
    for name, c in BLOCKS:
        conv(name + ".m_Block.0", c, c, 3, False)
        norm(name + ".m_Block.1", c)
        conv(name + ".m_Block.3", c, c, 3, False)
        norm(name + ".m_Block.4", c)
    conv("m_OutputLayer.0", 3, 32, 3, True, gain=8.0)
    return state


def flops_per_pixel(input_channels):
    """FLOPs per full-resolution output pixel, counted from the layer lists above: 2 x taps x Cin x Cout per output pixel
    of each layer, a layer at half resolution counting a quarter and so on. A transposed convolution spends 4 of its
    16 taps on each output pixel."""
    total, scale = 0.0, 1.0
    for name, cin, cout, stride in ENCODER:
        scale /= stride * stride
        total += scale * (9 * (cin or input_channels) * cout + 2 * 9 * cout * cout)  # the convolution and its block
    total += scale * 2 * 2 * 9 * 128 * 128  # the bottleneck's two blocks
    for name, cin, cout in DECODER:
        scale *= 4
        total += scale * (4 * cin * cout + 2 * 9 * cout * cout)
    total += 9 * 32 * 3
    return 2.0 * total


def forward_nchw(s, x, mirror=None, flip_transposed=None):
    """The network on an NCHW tensor `x`, `s` being a state_dict of x's dtype on x's device -> [N, 3, H, W]. `mirror`
    names one 3x3 convolution whose kernel is mirrored left to right, `flip_transposed` one transposed convolution whose
    kernel is flipped: the defects the tolerance has to tell from rounding."""
    def weight(prefix, flipped=False):
        w = s[prefix + ".weight"]
        if prefix == mirror:
            w = torch.flip(w, dims=[3])
        if flipped and prefix == flip_transposed:
            w = torch.flip(w, dims=[2, 3])
        return w

    def block(prefix, x):
        h = F.conv2d(x, weight(prefix + ".m_Block.0"), None, padding=1)
        h = F.batch_norm(h, s[prefix + ".m_Block.1.running_mean"], s[prefix + ".m_Block.1.running_var"],
                         s[prefix + ".m_Block.1.weight"], s[prefix + ".m_Block.1.bias"], False, 0.0, EPS)
        h = F.conv2d(F.relu(h), weight(prefix + ".m_Block.3"), None, padding=1)
        h = F.batch_norm(h, s[prefix + ".m_Block.4.running_mean"], s[prefix + ".m_Block.4.running_var"],
                         s[prefix + ".m_Block.4.weight"], s[prefix + ".m_Block.4.bias"], False, 0.0, EPS)
        return F.relu(h + x)

    def stage(prefix, x, stride):
        return block(prefix + ".2", F.relu(F.conv2d(x, weight(prefix + ".0"), s[prefix + ".0.bias"], stride=stride, padding=1)))

    def up(prefix, x):
        h = F.conv_transpose2d(x, weight(prefix + ".0", True), s[prefix + ".0.bias"], stride=2, padding=1)
        return block(prefix + ".2", F.relu(h))

    with torch.no_grad():
        skip1 = stage("m_EncoderStage1", x, 1)
        skip2 = stage("m_EncoderStage2", skip1, 2)
        h = stage("m_EncoderStage3", skip2, 2)
        h = block("m_Bottleneck.1", block("m_Bottleneck.0", h))
        h = up("m_DecodeStage2", h) + skip2
        h = up("m_DecodeStage1", h) + skip1
        return torch.sigmoid(F.conv2d(h, weight("m_OutputLayer.0"), s["m_OutputLayer.0.bias"], padding=1))


def forward(state, x_hwc, dtype=torch.float32, mirror=None, flip_transposed=None):
    """x_hwc: [H, W, C] array -> the network's [H, W, 3] output as a numpy array of `dtype`, on the CPU."""
    s = {k: v.to(dtype) for k, v in state.items() if v.is_floating_point()}
    x = torch.as_tensor(np.asarray(x_hwc)).to(dtype).permute(2, 0, 1)[None]
    return forward_nchw(s, x, mirror, flip_transposed)[0].permute(1, 2, 0).contiguous().numpy()


def container_bytes(state, input_channels, skip=()):
    """The weights container of a state_dict (the format: DESIGN 5k), written independently of the exporter tool.
    Integer tensors (num_batches_tracked) and the names in `skip` are left out."""
    named = [(k, v.detach().to(torch.float32).contiguous().numpy()) for k, v in state.items()
             if v.is_floating_point() and k not in skip]
    offset = HEADER_BYTES + ENTRY_BYTES * len(named)
    table, data = b"", b""
    for name, a in named:
        dims = list(a.shape) + [1] * (4 - a.ndim)
        raw = a.astype("<f4").tobytes()
        table += struct.pack("<64sI4IIQ", name.encode("ascii"), a.ndim, *dims, 0, offset + len(data))
        data += raw
    return MAGIC + struct.pack("<III12x", VERSION, input_channels, len(named)) + table + data


def pack_rgba8(hwc):
    """NormaliseAndReorderAiOutput + SubmitAiInterpolation's packing of an [H, W, C] tensor in [0, 1], float32: channels
    0 and 2 swapped when there are at least 3, clamp, round(v * 255.0f) half away from zero, alpha 255 (other missing
    channels 0) when absent -> uint8 [H, W, 4]."""
    v = np.asarray(hwc, np.float32)
    h, w, c = v.shape
    if c >= 3:
        v = v[..., [2, 1, 0] + list(range(3, c))]
    v = np.clip(v, np.float32(0), np.float32(1)) * np.float32(255)
    assert v.dtype == np.float32
    # half away from zero for v >= 0; v - floor(v) is exact in float32, which floor(v + 0.5) is not (0.49999997)
    r = np.where(v - np.floor(v) < np.float32(0.5), np.floor(v), np.floor(v) + 1)
    out = np.zeros((h, w, 4), np.uint8)
    out[..., 3] = 255
    out[..., :min(c, 4)] = r[..., :4].astype(np.uint8)
    return out
