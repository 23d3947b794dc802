#!/usr/bin/env python3
"""Convert a frame generator checkpoint into the weights container tri_framegen_create reads.

The checkpoint is what torch.save wrote: {"model_state": state_dict, ...} or a bare state_dict. Only named tensors
are copied, so no model class is needed: every floating-point tensor goes in as float32 under its state_dict key;
integer tensors (BatchNorm's num_batches_tracked) are left out. The input channels are read from the first
convolution, m_EncoderStage1.0.weight ([32, Cin, 3, 3]).

    tools/export_frame_generator.py checkpoint.pt Assets/AI/frame_generator.trifgen
"""
import argparse
import struct
import sys

import numpy as np

MAGIC, VERSION, HEADER_BYTES, ENTRY_BYTES, NAME_BYTES = b"TRIFGEN\0", 1, 32, 96, 64
EXTENSION = ".trifgen"
FIRST_LAYER = "m_EncoderStage1.0.weight"


def container_from_state(state):
    """state: {name: array-like or torch tensor} -> the container's bytes."""
    named = []
    for name, value in state.items():
        a = value.detach().cpu().numpy() if hasattr(value, "detach") else np.asarray(value)
        if not np.issubdtype(a.dtype, np.floating):
            continue
        if a.ndim < 1 or a.ndim > 4:
            raise ValueError(f"{name}: rank {a.ndim} outside 1..4")
        if len(name.encode("ascii")) >= NAME_BYTES:
            raise ValueError(f"{name}: the name does not fit {NAME_BYTES - 1} bytes")
        named.append((name, np.ascontiguousarray(a, dtype="<f4")))
    first = dict(named).get(FIRST_LAYER)
    if first is None or first.ndim != 4:
        raise ValueError(f"the checkpoint has no {FIRST_LAYER}: not a frame generator")
    offset = HEADER_BYTES + ENTRY_BYTES * len(named)
    table, data = [], []
    for name, a in named:
        dims = list(a.shape) + [1] * (4 - a.ndim)
        table.append(struct.pack("<64sI4IIQ", name.encode("ascii"), a.ndim, *dims, 0, offset))
        data.append(a.tobytes())
        offset += a.nbytes
    header = MAGIC + struct.pack("<III12x", VERSION, first.shape[1], len(named))
    return header + b"".join(table) + b"".join(data)


def read_container(blob):
    """The container's (input channels, {name: float32 array}) — the inverse of container_from_state."""
    if blob[:8] != MAGIC:
        raise ValueError("not a frame generator container")
    version, channels, count = struct.unpack_from("<III", blob, 8)
    if version != VERSION:
        raise ValueError(f"container version {version}")
    state = {}
    for i in range(count):
        name, rank, d0, d1, d2, d3, _, offset = struct.unpack_from("<64sI4IIQ", blob, HEADER_BYTES + ENTRY_BYTES * i)
        shape = (d0, d1, d2, d3)[:rank]
        n = int(np.prod(shape))
        state[name.rstrip(b"\0").decode("ascii")] = np.frombuffer(blob, "<f4", n, offset).reshape(shape).copy()
    return channels, state


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint", help="what torch.save wrote: {'model_state': ...} or a bare state_dict")
    ap.add_argument("output", help=f"the container to write (the renderer searches Assets/AI/frame_generator{EXTENSION})")
    args = ap.parse_args(argv)
    import torch

    loaded = torch.load(args.checkpoint, map_location="cpu")
    state = loaded["model_state"] if isinstance(loaded, dict) and "model_state" in loaded else loaded
    blob = container_from_state(state)
    with open(args.output, "wb") as f:
        f.write(blob)
    channels, tensors = read_container(blob)
    print(f"{args.output}: {len(tensors)} tensors, {channels} input channels, {len(blob)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
