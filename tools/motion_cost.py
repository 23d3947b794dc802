#!/usr/bin/env python3
"""What the motion-vector pass costs on one GPU, through the C-ABI: C2 (the 50k-triangle sphere) at
1920x1080 and C3 (the 1M-triangle grid) at 3840x2160, trains of tri_render with the id output on.

  1. motion off  frames per second of this tree with the motion output off and — with --parent-lib, a library built from
                 the parent commit — of the parent: the plan is launch for launch the parent's, so the tree's median must
                 lie inside the parent's own min-max spread;
  2. motion on   frames per second with the output on (a history with a moved camera and moved draws, so no row is the
                 identity), and the pass's time from events of its own (tri_set_timing stamps k_motion on both sides;
                 tri_get_motion_timing) against its traffic floor: 16 B per pixel (4 B id + 4 B depth read, 8 B motion
                 written) at the 6.3 TB/s a float4 copy reaches on one MI355X.
Every measurement runs in a fresh child process (one library per process); the children alternate between the parent's
library and this tree's, the variants alternate inside a child, and each figure is the median of the windows with the
min-max spread. Frame rates come from trains of tri_render on one stream timed by HIP events.

    python tools/motion_cost.py --out profiles/motion_cost.json [--parent-lib path/to/parent/libtri_raster.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-renderer_amd", "python"))

COPY_BYTES_PER_S = 6.3e12  # what a float4 copy reaches on one MI355X
BYTES_PER_PIXEL = 16


def stat(samples):
    return {"median": statistics.median(samples), "spread": [min(samples), max(samples)], "samples": samples}


def scene_list():
    from trident_raster import scenes

    return (("C2_1080p", scenes.scene_c2_sphere(1920, 1080)), ("C3_4K", scenes.scene_c3_grid(3840, 2160)))


def moved_history(scene):
    """A previous frame in which the camera and every draw lay elsewhere (a small translation of each)."""
    import numpy as np

    view = np.array(scene.ubo.view[:], np.float32)
    view[12] += 0.05
    view[13] -= 0.02
    models = np.array([d.pc.model[:] for d in scene.draws], np.float32).reshape(-1, 16)
    models[:, 12] += 0.03
    return view, np.array(scene.ubo.projection[:], np.float32), models


def measure(args, parent):
    """This process's library: {scene: {variant: figures}}. parent: a library without the motion entry points."""
    import torch

    if not torch.cuda.is_available():
        sys.exit("motion_cost.py measures on a GPU: none found")
    from trident_raster import raster, scenes

    raster.load_library()
    out = {"device": torch.cuda.get_device_name(0)}
    stream = torch.cuda.Stream()
    for name, scene in scene_list():
        with raster.TriRaster(scene.width, scene.height) as r:
            scenes.load_scene(r, scene)
            r.set_stream(stream.cuda_stream)
            r.set_id_output(True)
            if not parent:
                hist = moved_history(scene)

            def setup(variant):
                if parent:
                    return
                r.set_motion_output(variant == "on")
                if variant == "on":
                    r.set_motion_history(*hist)

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
                mo_ms, mo_frames = r.motion_timing()
                r.set_timing(False)
                us = {k[3:] + "_us": 1e3 * t[k] / t["frames"] for k in ("ms_vertex", "ms_setup", "ms_raster", "ms_frame")}
                us["motion_us"] = 1e3 * mo_ms / mo_frames if mo_frames else 0.0
                return us

            variants = ["off"] if parent else ["off", "on"]
            fps = {v: [] for v in variants}
            for v in variants:
                window(v, 10)
            for _ in range(args.windows):
                for v in variants:
                    fps[v].append(window(v, args.frames))
            entry = {v: {"fps": stat(fps[v])} for v in variants}
            if not parent:
                entry["stage_us"] = {v: stages(v, args.frames) for v in variants}
                assert bool(r.read_motion().any()), "the measured frames carried no motion"
            out[name] = entry
    return out


def child(args, which):
    env = dict(os.environ)
    if which == "parent":
        env["TRI_RASTER_LIB"] = os.path.abspath(args.parent_lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--windows", str(args.windows),
                        "--frames", str(args.frames)], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.exit(f"motion_cost.py: the {which} child failed:\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
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
    result = {"frames_per_window": args.frames, "windows": args.windows, "rounds": args.rounds,
              "device": runs["tree"][0]["device"], "copy_bytes_per_s": COPY_BYTES_PER_S}
    for name, scene in ((n, s) for n, s in scene_list()):
        def pooled(which, variant):
            return stat([s for run in runs[which] for s in run[name][variant]["fps"]["samples"]])

        def stage(variant, key):
            return stat([run[name]["stage_us"][variant][key] for run in runs["tree"]])

        pixels = scene.width * scene.height
        floor_us = 1e6 * pixels * BYTES_PER_PIXEL / COPY_BYTES_PER_S
        off, on = pooled("tree", "off"), pooled("tree", "on")
        motion_us = stage("on", "motion_us")
        entry = {
            "pixels": pixels, "traffic_bytes": pixels * BYTES_PER_PIXEL, "traffic_floor_us": floor_us,
            "motion_off_fps": off, "motion_on_fps": on,
            "motion_added_us_per_frame": 1e6 / on["median"] - 1e6 / off["median"],
            "motion_pass_us": motion_us,
            "motion_pass_bytes_per_s": pixels * BYTES_PER_PIXEL / (motion_us["median"] * 1e-6),
            "motion_pass_fraction_of_copy_rate": floor_us / motion_us["median"],
            "raster_us_motion_on": stage("on", "raster_us"), "raster_us_motion_off": stage("off", "raster_us"),
            "frame_us_motion_on": stage("on", "frame_us"), "frame_us_motion_off": stage("off", "frame_us"),
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
