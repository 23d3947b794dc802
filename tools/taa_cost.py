#!/usr/bin/env python3
"""What the temporal anti-aliasing pass costs on one GPU, through the C-ABI, by tools/reproject_cost.py's
method: C2 (the 50k-triangle sphere) at 1920x1080 and C3 (the 1M-triangle grid) at 3840x2160, trains of tri_render on
one stream with the id output on.

  1. no taa   frames per second of this tree with no tri_taa in use and — with --parent-lib, a library built from the
              parent commit — of the parent: no kernel and no launch plan changed, so the tree's median must lie inside
              the parent's own min-max spread;
  2. motion   frames per second with the motion output on (a moved camera and moved draws), the pass's precondition;
  3. taa      frames per second with tri_taa_resolve behind every tri_render, and the pass's own time from the object's
              events (tri_set_timing; tri_taa_get_timing; one render, one pass, one wait per sample) against its traffic
              floor: 41 B per pixel — 12 B of the current frame read (colour, id, depth), 8 B of history read, 8 + 4 B of
              history written, 4 + 1 B of resolved colour and mask written, 4 B of previous ids under the id test — at the
              6.3 TB/s a float4 copy reaches on one MI355X;
  4. the yardstick  k_reproject<4> (tri_history_reproject) behind the SAME frames in the SAME samples, from its own
              object's events: the pass the issue compares k_taa_resolve with.
The frames of 3 and 4 are rendered under the jitter contract (tri_taa_jitter, period 8). Every measurement runs in a
fresh child process (one library per process); the children alternate between the parent's library and this tree's, the
variants alternate inside a child, and each figure is the median of the windows with the min-max spread.

    python tools/taa_cost.py --out profiles/taa_cost.json [--parent-lib path/to/parent/libtri_raster.so]
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
PERIOD, ALPHA = 8, 0.1


def stat(samples):
    return {"median": statistics.median(samples), "spread": [min(samples), max(samples)], "samples": samples}


def measure(args, parent):
    """This process's library: {scene: {variant: figures}}. parent: a library without the tri_taa entry points."""
    import numpy as np
    import torch

    from motion_cost import moved_history, scene_list

    if not torch.cuda.is_available():
        sys.exit("taa_cost.py measures on a GPU: none found")
    from trident_raster import abi, raster, scenes

    raster.load_library()
    out = {"device": torch.cuda.get_device_name(0)}
    stream = torch.cuda.Stream()
    for name, scene in scene_list():
        with raster.TriRaster(scene.width, scene.height) as r:
            scenes.load_scene(r, scene)
            r.set_stream(stream.cuda_stream)
            r.set_id_output(True)
            hist = moved_history(scene)
            taa = None if parent else raster.TriTaa(scene.width, scene.height)
            history = None if parent else raster.TriHistory(scene.width, scene.height)
            proj = np.array(scene.ubo.projection[:], np.float32)

            def set_jittered(index):
                """Frame `index` under the jitter contract: the jittered block, the previous projection under the same jitter."""
                jx, jy = raster.taa_jitter(index, PERIOD)
                ubo = abi.TriGlobalUbo.from_buffer_copy(scene.ubo)
                ubo.projection = (abi.C.c_float * 16)(*raster.taa_jitter_projection(proj, jx, jy, scene.width, scene.height).tolist())
                r.set_frame(ubo, scene.clear)
                r.set_motion_history(hist[0], raster.taa_jitter_projection(hist[1], jx, jy, scene.width, scene.height), hist[2])

            def setup(variant):
                if parent:
                    return
                r.set_frame(scene.ubo, scene.clear)
                r.set_motion_output(variant != "off")
                if variant != "off":
                    r.set_motion_history(*hist)

            def window(variant, frames):
                setup(variant)
                r.render_frame()  # switches and buffer growth happen outside the timed window
                if variant == "taa":
                    taa.resolve(r, ALPHA)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(frames):
                    r.render()
                    if variant == "taa":
                        taa.resolve(r, ALPHA)
                e1.record(stream)
                r.synchronize()
                return frames / (e0.elapsed_time(e1) * 1e-3)

            def pass_us(frames):
                """(k_taa_resolve, k_reproject<4>) microseconds per sample, both behind the same jittered frame."""
                setup("taa")
                set_jittered(0)
                r.render_frame()
                taa.resolve(r, ALPHA)
                history.reproject(r)
                r.synchronize()
                t0, h0 = taa.timing(), history.timing()
                r.set_timing(True)
                ours, theirs = [], []
                for k in range(frames):
                    set_jittered(k + 1)
                    r.render()
                    if k % 2:  # the two passes alternate places behind the frame
                        taa.resolve(r, ALPHA)
                        history.reproject(r)
                    else:
                        history.reproject(r)
                        taa.resolve(r, ALPHA)
                    r.synchronize()
                    t1, h1 = taa.timing(), history.timing()
                    assert t1[1] == t0[1] + 1 and h1[1] == h0[1] + 1
                    ours.append(1e3 * (t1[0] - t0[0]))
                    theirs.append(1e3 * (h1[0] - h0[0]))
                    t0, h0 = t1, h1
                r.set_timing(False)
                return ours, theirs

            variants = ["off"] if parent else ["off", "motion", "taa"]
            fps = {v: [] for v in variants}
            for v in variants:
                window(v, 10)
            for _ in range(args.windows):
                for v in variants:
                    fps[v].append(window(v, args.frames))
            entry = {v: {"fps": stat(fps[v])} for v in variants}
            if not parent:
                entry["taa_pass_us"], entry["reproject_pass_us"] = pass_us(args.frames)
                _, _, mask = taa.read()
                entry["valid_fraction"] = float(((mask & 15) == 0).mean())
                entry["clamped_fraction"] = float(((mask & abi.TRI_TAA_CLAMPED) != 0).mean())
                taa.close()
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
        sys.exit(f"taa_cost.py: the {which} child failed:\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def brief(t):
    return {"median": t["median"], "spread": t["spread"], "count": len(t["samples"])}


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
            print(f"taa_cost.py: {which} child {len(runs[which])} of {args.rounds} done", file=sys.stderr, flush=True)
    result = {"frames_per_window": args.frames, "windows": args.windows, "rounds": args.rounds,
              "device": runs["tree"][0]["device"], "copy_bytes_per_s": COPY_BYTES_PER_S, "bytes_per_pixel": BYTES_PER_PIXEL,
              "jitter_period": PERIOD, "alpha": ALPHA}
    for name, scene in scene_list():
        def pooled(which, variant):
            return stat([s for run in runs[which] for s in run[name][variant]["fps"]["samples"]])

        pixels = scene.width * scene.height
        floor_us = 1e6 * pixels * BYTES_PER_PIXEL / COPY_BYTES_PER_S
        off, motion, taa = pooled("tree", "off"), pooled("tree", "motion"), pooled("tree", "taa")
        ours = stat([s for run in runs["tree"] for s in run[name]["taa_pass_us"]])
        theirs = stat([s for run in runs["tree"] for s in run[name]["reproject_pass_us"]])
        entry = {
            "pixels": pixels, "traffic_bytes": pixels * BYTES_PER_PIXEL, "traffic_floor_us": floor_us,
            "no_taa_fps": off, "motion_fps": motion, "taa_fps": taa,
            "taa_added_us_per_frame": 1e6 / taa["median"] - 1e6 / motion["median"],
            "taa_pass_us": brief(ours),
            "taa_pass_bytes_per_s": pixels * BYTES_PER_PIXEL / (ours["median"] * 1e-6),
            "taa_pass_fraction_of_copy_rate": floor_us / ours["median"],
            "reproject_pass_us_same_run": brief(theirs),
            "taa_over_reproject": ours["median"] / theirs["median"],
            "taa_slower_than_reproject_beyond_spread": ours["median"] > theirs["spread"][1],
            "valid_fraction": statistics.median(run[name]["valid_fraction"] for run in runs["tree"]),
            "clamped_fraction": statistics.median(run[name]["clamped_fraction"] for run in runs["tree"]),
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
