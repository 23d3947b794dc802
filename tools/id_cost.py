#!/usr/bin/env python3
"""What the entity-id pass costs on one GPU, through the C-ABI: C2 (the 50k-triangle sphere) at
1920x1080 and C3 (the 1M-triangle grid) at 3840x2160.

  1. ids off    frames per second of this tree with the id output off, and — with --parent-lib, a library built from the
                parent commit — of the parent, in alternating child processes (one library per process): the plan and
                the kernels are unchanged, so the two must agree within the parent's own run-to-run spread;
  2. ids on     frames per second with the output on, and the pass's time from events of its own (tri_set_timing stamps
                k_id_raster on both sides; tri_get_id_timing), beside the stages of the same frames: ms_raster, and
                ms_setup, which no longer contains the pass;
  3. single calls at C3's extent: one tri_pick and one full-frame tri_pick_rect (host wall clock of the synchronous call
                on an idle context), and the outline pass at width 2 (frame time with the outline minus without).
Frame rates come from trains of tri_render on one stream timed by HIP events; the variants alternate, each figure is the
median of the windows with the spread.

    python tools/id_cost.py --out profiles/id_cost.json [--parent-lib path/to/parent/libtri_raster.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-renderer_amd", "python"))


def stat(samples):
    return {"median": statistics.median(samples), "spread": [min(samples), max(samples)], "samples": samples}


def scene_list():
    from trident_raster import scenes

    return (("C2_1080p", scenes.scene_c2_sphere(1920, 1080)), ("C3_4K", scenes.scene_c3_grid(3840, 2160)))


def measure(args, ids_off_only):
    """This process's library: {scene: {variant: figures}}. ids_off_only: a library without the id entry points."""
    import torch

    if not torch.cuda.is_available():
        sys.exit("id_cost.py measures on a GPU: none found")
    from trident_raster import raster, scenes

    raster.load_library()
    out = {"device": torch.cuda.get_device_name(0)}
    stream = torch.cuda.Stream()
    for name, scene in scene_list():
        with raster.TriRaster(scene.width, scene.height) as r:
            scenes.load_scene(r, scene)
            r.set_stream(stream.cuda_stream)

            def setup(variant):
                if ids_off_only:
                    return
                r.set_id_output(variant != "off")  # (off also removes the outline)
                if variant != "off":
                    r.set_outline([0] if variant == "outline" else None, (1.0, 0.6, 0.0, 1.0), 2)

            def window(variant, frames):
                setup(variant)
                r.render_frame()  # switches and buffer growth happen outside the timed window
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(frames):
                    r.render()
                e1.record(stream)
                r.synchronize()
                return frames / (e0.elapsed_time(e1) * 1e-3)

            def stages(variant, frames):
                setup(variant)
                r.render_frame()
                r.set_timing(True)
                for _ in range(frames):
                    r.render()
                t = r.timing()
                id_ms, id_frames = r.id_timing()
                r.set_timing(False)
                us = {k[3:] + "_us": 1e3 * t[k] / t["frames"] for k in ("ms_vertex", "ms_setup", "ms_raster", "ms_frame")}
                us["id_us"] = 1e3 * id_ms / id_frames if id_frames else 0.0
                return us

            variants = ["off"] if ids_off_only else ["off", "on", "outline"]
            fps = {v: [] for v in variants}
            for v in variants:
                window(v, 10)
            for _ in range(args.windows):
                for v in variants:
                    fps[v].append(window(v, args.frames))
            entry = {v: {"fps": stat(fps[v])} for v in variants}
            if not ids_off_only:
                st = {v: stages(v, args.frames) for v in ("off", "on")}
                entry["stage_us"] = st
                entry["id_pass_us"] = st["on"]["id_us"]
                entry["raster_us"] = st["on"]["raster_us"]
                off, on, line = (1e6 / entry[v]["fps"]["median"] for v in ("off", "on", "outline"))
                entry["ids_added_us_per_frame"] = on - off
                entry["outline_added_us_per_frame"] = line - on
                # single calls on an idle context
                setup("on")
                r.render_frame()
                picks, rects = [], []
                for k in range(args.windows * 3):
                    t0 = time.perf_counter()
                    r.pick(scene.width // 2 + k, scene.height // 2)
                    picks.append(1e6 * (time.perf_counter() - t0))
                    t0 = time.perf_counter()
                    r.pick_rect(0, 0, scene.width - 1, scene.height - 1, 1)
                    rects.append(1e6 * (time.perf_counter() - t0))
                entry["pick_us"] = stat(picks)
                entry["pick_rect_full_frame_us"] = stat(rects)
            out[name] = entry
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--frames", type=int, default=60, help="frames per window")
    ap.add_argument("--rounds", type=int, default=3, help="alternating child processes per library (with --parent-lib)")
    ap.add_argument("--parent-lib", default=None, help="libtri_raster.so built from the parent commit")
    ap.add_argument("--child", choices=["tree", "parent"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:  # one library, ids off, one JSON line
        print(json.dumps(measure(args, True)))
        return
    result = {"frames_per_window": args.frames, "windows": args.windows, "tree": measure(args, False)}
    if args.parent_lib:
        # one library per process: children alternate between this tree's library and the parent's, ids off in both
        runs = {"tree": [], "parent": []}
        for _ in range(args.rounds):
            for which in ("parent", "tree"):
                env = dict(os.environ)
                if which == "parent":
                    env["TRI_RASTER_LIB"] = os.path.abspath(args.parent_lib)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--windows", str(args.windows),
                                    "--frames", str(args.frames)], env=env, capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    sys.exit(f"id_cost.py: the {which} child failed:\n{p.stderr[-2000:]}")
                runs[which].append(json.loads(p.stdout.strip().splitlines()[-1]))
        pairs = {}
        for name, _ in scene_list():
            pairs[name] = {w: stat([s for run in runs[w] for s in run[name]["off"]["fps"]["samples"]]) for w in runs}
            lo, hi = pairs[name]["parent"]["spread"]
            pairs[name]["tree_median_inside_parent_spread"] = lo <= pairs[name]["tree"]["median"] <= hi
        result["ids_off_tree_vs_parent_fps"] = pairs
    print(json.dumps(result, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
