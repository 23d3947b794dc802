"""The dataset-capture tests' yardstick, restated in numpy from the reference's host code:

- the AI input tensor (ResolvePendingReadback, Renderer.cpp:1111-1389): float(byte) * (1.0f / 255.0f), one float32
  multiply by the float32 constant 0x3B808081, the B8G8R8A8 bytes reordered {2, 1, 0, 3};
- the NPY 1.0 bytes and the metadata text of AI::FrameDatasetRecorder (FrameDatasetRecorder.cpp:275-366): the
  preamble padded to a multiple of 16 (np.save pads to 64; np.load reads both);
- NormaliseAndReorderAiOutput (Renderer.cpp:358-415) and the output-shape rules (FrameDatasetRecorder.cpp:164-176)."""
import struct

import numpy as np

INV255 = np.float32(1) / np.float32(255)
assert INV255.view(np.uint32) == 0x3B808081


def unorm_table():
    """float32 [256]: the tensor value of every byte."""
    return np.arange(256, dtype=np.uint8).astype(np.float32) * INV255


def tensor_from_bgra(bgra):
    """uint8 [..., 4] in memory order B, G, R, A -> float32 [..., 4] in R, G, B, A."""
    bgra = np.asarray(bgra, np.uint8)
    return bgra[..., [2, 1, 0, 3]].astype(np.float32) * INV255


def tensor_from_rgba(rgba):
    """uint8 [..., 4] RGBA (what ReadViewportPixels returns) -> float32 [..., 4]."""
    return np.asarray(rgba, np.uint8).astype(np.float32) * INV255


def division_variant(byte_values):
    """What a division by 255 would give instead (it differs on 126 of the 256 byte values)."""
    return np.asarray(byte_values, np.uint8).astype(np.float32) / np.float32(255)


def shape_string(shape):
    s = "(" + ", ".join(str(int(d)) for d in shape)
    return s + (",)" if len(shape) == 1 else ")")


def npy_bytes(data, shape):
    """The file WriteNpyFile writes for float32 `data` with `shape`."""
    header = "{'descr': '<f4', 'fortran_order': False, 'shape': " + shape_string(shape) + ", }"
    header += " " * ((16 - (10 + len(header) + 1) % 16) % 16) + "\n"
    payload = np.ascontiguousarray(data, "<f4").tobytes()
    return b"\x93NUMPY\x01\x00" + struct.pack("<H", len(header)) + header.encode("ascii") + payload


def metadata_text(width, height, channels, shape):
    """The metadata file of an input sample. colorOrder reads BGRA although the tensor is RGBA: the reference's own
    label (FrameDatasetRecorder.cpp:121), kept byte for byte."""
    layout = '  "layout": "%s",\n' % shape_string(shape) if len(shape) else ""
    return ('{\n  "width": %d,\n  "height": %d,\n  "channels": %d,\n%s  "channelsLast": true,\n'
            '  "colorOrder": "BGRA",\n  "normalised": true\n}\n' % (width, height, channels, layout))


def output_shape(shape, count):
    """RecordAiOutput's shape normalisation: no shape -> (count,); rank 3 gets a leading 1; rank >= 4 a batch >= 1;
    rank 1 -> (1, n, 1, 1)."""
    shape = [int(d) for d in shape] if len(shape) else [int(count)]
    if len(shape) == 3:
        return [1] + shape
    if len(shape) >= 4:
        return [1 if shape[0] <= 0 else shape[0]] + shape[1:]
    if len(shape) == 1:
        return [1, shape[0], 1, 1]
    return shape


def normalise_ai_output(data, channels):
    """NormaliseAndReorderAiOutput on a flat float32 array of whole pixels: scale by float32(1/255) when max > 1 + 1e-3
    or min < -1e-3 (float32 comparisons), swap channels 0 and 2 when channels >= 3, clamp to [0, 1]."""
    v = np.array(data, np.float32).reshape(-1)
    tol = np.float32(1.0e-3)
    if v.max() > np.float32(1) + tol or v.min() < -tol:
        v = v * INV255
    if channels >= 3:
        px = v.reshape(-1, channels)
        px[:, [0, 2]] = px[:, [2, 0]]
        v = px.reshape(-1)
    return np.clip(v, np.float32(0), np.float32(1)).astype(np.float32)
