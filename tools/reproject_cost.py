#!/usr/bin/env python3
"""What the history reprojection pass costs on one GPU, through the C-ABI, by tools/motion_cost.py's
method: C2 (the 50k-triangle sphere) at 1920x1080 and C3 (the 1M-triangle grid) at 3840x2160, trains of tri_render on
one stream with the id output on.

  1. no history  frames per second of this tree with no tri_history in use and — with --parent-lib, a library built from
                 the parent commit — of the parent: no kernel and no launch plan changed, so the tree's median must lie
                 inside the parent's own min-max spread;
  2. motion      frames per second with the motion output on (a moved camera and moved draws), the pass's precondition;
  3. reproject   frames per second with tri_history_reproject behind every tri_render, and the pass's own time from the
                 object's events (tri_set_timing; tri_history_get_timing; one render, one pass, one wait per sample)
                 against its traffic floor: 41 B per pixel — 12 B of the current frame read, 12 B of the previous frame
                 read, 4 + 1 B of warped colour and mask written, 12 B of history written — at the 6.3 TB/s a float4
                 copy reaches on one MI355X; and the same under caller-bound targets that are not 16-B aligned, which
                 take the one-pixel-per-lane kernel.
Every measurement runs in a fresh child process (one library per process); the children alternate between the parent's
library and this tree's, the variants alternate inside a child, and each figure is the median of the windows with the
min-max spread.

    python tools/reproject_cost.py --out profiles/reproject_cost.json [--parent-lib path/to/parent/libtri_raster.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_BYTES_PER_S = 6.3e12  # what a float4 copy reaches on one MI355X
BYTES_PER_PIXEL = 41


def stat(samples):
    return {"median": statistics.median(samples), "spread": [min(samples), max(samples)], "samples": samples}


def measure(args, parent):
    """This process's library: {scene: {variant: figures}}. parent: a library without the history entry points."""
    import torch

    from motion_cost import moved_history, scene_list

    if not torch.cuda.is_available():
        sys.exit("reproject_cost.py measures on a GPU: none found")
    from trident_raster import raster, scenes

    raster.load_library()
    out = {"device": torch.cuda.get_device_name(0)}
    stream = torch.cuda.Stream()
    for name, scene in scene_list():
        with raster.TriRaster(scene.width, scene.height) as r:
            scenes.load_scene(r, scene)
            r.set_stream(stream.cuda_stream)
            r.set_id_output(True)
            hist = moved_history(scene)
            history = None if parent else raster.TriHistory(scene.width, scene.height)

            def setup(variant):
                if parent:
                    return
                r.set_motion_output(variant != "off")
                if variant != "off":
                    r.set_motion_history(*hist)

            def window(variant, frames):
                setup(variant)
                r.render_frame()  # switches and buffer growth happen outside the timed window
                if variant == "reproject":
                    history.reproject(r)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(frames):
                    r.render()
                    if variant == "reproject":
                        history.reproject(r, 1e-3)
                e1.record(stream)
                r.synchronize()
                return frames / (e0.elapsed_time(e1) * 1e-3)

            def pass_us(frames):
                setup("reproject")
                r.render_frame()
                history.reproject(r, 1e-3)
                r.synchronize()
                ms0, n0 = history.timing()
                r.set_timing(True)
                samples = []
                for _ in range(frames):
                    r.render()
                    history.reproject(r, 1e-3)
                    r.synchronize()
                    ms1, n1 = history.timing()
                    assert n1 == n0 + 1
                    samples.append(1e3 * (ms1 - ms0))
                    ms0, n0 = ms1, n1
                r.set_timing(False)
                return samples

            variants = ["off"] if parent else ["off", "motion", "reproject"]
            fps = {v: [] for v in variants}
            for v in variants:
                window(v, 10)
            for _ in range(args.windows):
                for v in variants:
                    fps[v].append(window(v, args.frames))
            entry = {v: {"fps": stat(fps[v])} for v in variants}
            if not parent:
                entry["pass_us"] = pass_us(args.frames)
                # the same frames rendered into caller-bound targets 4 B past a 16-B boundary: one pixel per lane
                n = scene.width * scene.height
                col = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
                dep = torch.zeros(n + 1, dtype=torch.float32, device="cuda:0")
                torch.cuda.synchronize()
                r.bind_output(col[1:].data_ptr(), dep[1:].data_ptr())
                entry["pass_us_one_pixel_per_lane"] = pass_us(args.frames)
                r.bind_output(None, None)
                _, mask = history.read()
                entry["valid_fraction"] = float((mask == 0).mean())
                history.close()
            out[name] = entry
    return out


def child(args, which):
    env = dict(os.environ)
    if which == "parent":
        env["TRI_RASTER_LIB"] = os.path.abspath(args.parent_lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--windows", str(args.windows),
                        "--frames", str(args.frames)], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.exit(f"reproject_cost.py: the {which} child failed:\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    from motion_cost import scene_list

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--frames", type=int, default=60, help="frames per window")
    ap.add_argument("--rounds", type=int, default=3, help="alternating child processes per library")
    ap.add_argument("--parent-lib", default=None, help="libtri_raster.so built from the parent commit")
    ap.add_argument("--child", choices=["tree", "parent"], default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.child:  # one library, one JSON line
        print(json.dumps(measure(args, args.child == "parent")))
        return
    runs = {"tree": [], "parent": []}
    for _ in range(args.rounds):
        for which in (("parent", "tree") if args.parent_lib else ("tree",)):
            runs[which].append(child(args, which))
            print(f"reproject_cost.py: {which} child {len(runs[which])} of {args.rounds} done", file=sys.stderr, flush=True)
    result = {"frames_per_window": args.frames, "windows": args.windows, "rounds": args.rounds,
              "device": runs["tree"][0]["device"], "copy_bytes_per_s": COPY_BYTES_PER_S, "bytes_per_pixel": BYTES_PER_PIXEL}
    for name, scene in scene_list():
        def pooled(which, variant):
            return stat([s for run in runs[which] for s in run[name][variant]["fps"]["samples"]])

        pixels = scene.width * scene.height
        floor_us = 1e6 * pixels * BYTES_PER_PIXEL / COPY_BYTES_PER_S
        off, motion, rep = pooled("tree", "off"), pooled("tree", "motion"), pooled("tree", "reproject")
        pass_us = stat([s for run in runs["tree"] for s in run[name]["pass_us"]])
        entry = {
            "pixels": pixels, "traffic_bytes": pixels * BYTES_PER_PIXEL, "traffic_floor_us": floor_us,
            "no_history_fps": off, "motion_fps": motion, "reproject_fps": rep,
            "reproject_added_us_per_frame": 1e6 / rep["median"] - 1e6 / motion["median"],
            "reproject_pass_us": {"median": pass_us["median"], "spread": pass_us["spread"], "count": len(pass_us["samples"])},
            "reproject_pass_bytes_per_s": pixels * BYTES_PER_PIXEL / (pass_us["median"] * 1e-6),
            "reproject_pass_fraction_of_copy_rate": floor_us / pass_us["median"],
            "reproject_pass_us_one_pixel_per_lane": (lambda t: {"median": t["median"], "spread": t["spread"], "count": len(t["samples"])})(
                stat([s for run in runs["tree"] for s in run[name]["pass_us_one_pixel_per_lane"]])),
            "valid_fraction": statistics.median(run[name]["valid_fraction"] for run in runs["tree"]),
        }
        if args.parent_lib:
            par = pooled("parent", "off")
            entry["parent_fps"] = par
            entry["tree_median_inside_parent_spread"] = par["spread"][0] <= off["median"] <= par["spread"][1]
        result[name] = entry
    print(json.dumps(result, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
