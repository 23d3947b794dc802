#!/usr/bin/env python3
"""What the text overlay pass costs on one GPU, through the C-ABI: C3 (the 1M-triangle grid) at 3840x2160 with
  (a) none     no text (tri_render enqueues exactly the frame's own launches);
  (b) label    the Forge Game viewport's label "FPS: 123.4" at (10, 30), 10 glyphs of the default 32-pixel font;
  (c) console  a full page, 64 lines x 200 characters = 12,800 glyphs.
Device time per frame from HIP events around trains of tri_render on one stream (frames back to back, no host wait
inside a train); the variants alternate and repeat, the median is reported with the spread. (b) and (c) are also given
as added microseconds over (a) and against the HBM bound on the bytes the pass must move: the colour read and written
over the 32 x 32 screen bins the quads touch, plus the atlas once (6.3 TB/s, the rate a float4 copy reaches).
(a) is the figure to compare with the parent commit's C3 frame on the same box: run this script there with
--variants none (it then needs nothing the parent lacks).

    python tools/text_cost.py --font tests/golden/fonts/JetBrainsMono-Regular.ttf --out profiles/round9/text_cost.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-renderer_amd", "python"))

HBM_BYTES_PER_S = 6.3e12
W, H = 3840, 2160


def page_text():
    line = "".join(chr(33 + (7 * i) % 94) for i in range(200))
    return "\n".join(line[k % 50:] + line[:k % 50] for k in range(64))


def pass_bytes(quads, bin_px=32):
    """Colour bytes read + written over the screen bins the quads touch (clipped to the frame)."""
    import numpy as np

    touched = np.zeros(((H + bin_px - 1) // bin_px, (W + bin_px - 1) // bin_px), bool)
    for q in quads:
        x0, x1 = sorted((q[0], q[2]))
        y0, y1 = sorted((q[1], q[3]))
        bx0, bx1 = int(max(x0, 0)) // bin_px, int(min(x1, W - 1)) // bin_px
        by0, by1 = int(max(y0, 0)) // bin_px, int(min(y1, H - 1)) // bin_px
        if x1 > 0 and y1 > 0 and x0 < W and y0 < H:
            touched[by0:by1 + 1, bx0:bx1 + 1] = True
    return int(touched.sum()) * bin_px * bin_px * 8


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--font", default=os.path.join(ROOT, "tests", "golden", "fonts", "JetBrainsMono-Regular.ttf"))
    ap.add_argument("--variants", default="none,label,console")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, default=40, help="frames per train")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("text_cost.py measures on a GPU: none found")
    from trident_raster import raster, scenes

    raster.load_library()
    variants = args.variants.split(",")
    quads, atlas = {"none": None}, None
    if any(v != "none" for v in variants):
        from trident_raster import app

        font = app.Font(args.font, 32.0)
        atlas = font.atlas()
        quads["label"] = font.layout("FPS: 123.4", (10.0, 30.0))
        quads["console"] = font.layout(page_text(), (8.0, 30.0))
        assert len(quads["console"]) == 12800, len(quads["console"])
    scene = scenes.scene_c3_grid(W, H)
    stream = torch.cuda.Stream()
    result = {"device": torch.cuda.get_device_name(0), "width": W, "height": H, "frames_per_train": args.frames,
              "repeats": args.repeats, "variants": {}}
    with raster.TriRaster(W, H) as r:
        scenes.load_scene(r, scene)
        r.set_stream(stream.cuda_stream)
        font_dev = raster.TriFont(atlas) if atlas is not None else None
        samples = {v: [] for v in variants}

        def train(v, frames):
            if font_dev is not None:
                r.set_text(font_dev if quads[v] is not None else None, quads[v])
            r.render_frame()  # the upload and any buffer growth happen outside the timed train
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(frames):
                r.render()
            e1.record(stream)
            r.synchronize()
            return e0.elapsed_time(e1) * 1e3 / frames  # microseconds per frame

        for v in variants:
            train(v, 10)
        for _ in range(args.repeats):  # alternating trains
            for v in variants:
                samples[v].append(train(v, args.frames))
        if font_dev is not None:
            r.set_text(None, None)
            font_dev.close()
    base = statistics.median(samples["none"]) if "none" in samples else None
    for v in variants:
        s = samples[v]
        entry = {"us_per_frame": statistics.median(s), "us_per_frame_spread": [min(s), max(s)], "samples": s}
        if v != "none":
            entry["glyphs"] = int(len(quads[v]))
            entry["pass_bytes"] = pass_bytes(quads[v]) + int(atlas.size)
            entry["hbm_bound_us"] = entry["pass_bytes"] / HBM_BYTES_PER_S * 1e6
            if base is not None:
                entry["added_us"] = entry["us_per_frame"] - base
                entry["hbm_bound_fraction"] = entry["hbm_bound_us"] / entry["added_us"] if entry["added_us"] > 0 else None
        result["variants"][v] = entry
    print(json.dumps(result, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
