#!/usr/bin/env python3
"""What temporal upscaling costs on one GPU, through the C-ABI, by tools/taa_cost.py's method, on C3's
geometry (the 1M-triangle grid), trains of tri_render on one stream with the id output on, in the same run:

  1. taa_4k      a 3840x2160 render with tri_taa_resolve behind every tri_render (§5p's anti-aliased 4K frame);
  2. up_1080p    a 1920x1080 render with tri_upscale_resolve to 3840x2160 behind every tri_render;
  3. up_1440p    a 2560x1440 render upscaled to 3840x2160;
  4. off         this tree's raw 3840x2160 frame with no tri_upscale (and no tri_taa) in use and — with --parent-lib, a
                 library built from the parent commit — the parent's: no kernel and no launch plan changed, so the tree's
                 median should lie inside the parent's own min-max spread.
Per chain: frames per second of the whole chain (render + pass) and the pass's own time from its object's events
(tri_set_timing; one render, one pass, one wait per sample; for tri_upscale the interval covers the kernel and the id
copy) against its traffic floor at the 6.3 TB/s a float4 copy reaches on one MI355X. The floor of the upscale rule: 21 B
per OUTPUT pixel (8 B of history read, 8 B written, 4 + 1 B of resolved colour and mask written) plus 20 B per RENDER pixel
(12 B of the current frame read — colour, id, depth —, 4 B of previous ids under the id test, 4 B of ids written); tri_taa's
is 41 B per pixel. The frames are rendered under the jitter contract with a moved camera and moved draws. Every
measurement runs in a fresh child process (one library per process); the children alternate between the parent's
library and this tree's, the chains alternate inside a child, and each figure is the median with the min-max spread.

    python tools/upscale_cost.py --out profiles/upscale_cost.json [--parent-lib path/to/parent/libtri_raster.so]
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
OUT_W, OUT_H = 3840, 2160
BYTES_PER_OUTPUT_PIXEL, BYTES_PER_RENDER_PIXEL, TAA_BYTES_PER_PIXEL = 21, 20, 41
ALPHA = 0.1
CHAINS = (("taa_4k", 3840, 2160), ("up_1080p", 1920, 1080), ("up_1440p", 2560, 1440))


def stat(samples):
    return {"median": statistics.median(samples), "spread": [min(samples), max(samples)], "samples": samples}


def floor_bytes(name, rw, rh):
    if name == "taa_4k":
        return TAA_BYTES_PER_PIXEL * rw * rh
    return BYTES_PER_OUTPUT_PIXEL * OUT_W * OUT_H + BYTES_PER_RENDER_PIXEL * rw * rh


def measure(args, parent):
    """This process's library: {chain: figures}. parent: a library without the tri_upscale entry points — `off` only."""
    import numpy as np
    import torch

    from motion_cost import moved_history

    if not torch.cuda.is_available():
        sys.exit("upscale_cost.py measures on a GPU: none found")
    from trident_raster import abi, raster, scenes

    raster.load_library()
    out = {"device": torch.cuda.get_device_name(0)}
    stream = torch.cuda.Stream()

    class Chain:
        def __init__(self, name, rw, rh):
            self.name, self.scene = name, scenes.scene_c3_grid(rw, rh)
            self.r = raster.TriRaster(rw, rh)
            scenes.load_scene(self.r, self.scene)
            self.r.set_stream(stream.cuda_stream)
            self.r.set_id_output(True)
            self.hist = moved_history(self.scene)
            self.proj = np.array(self.scene.ubo.projection[:], np.float32)
            self.obj, self.period = None, 8
            if name == "taa_4k":
                self.obj = raster.TriTaa(rw, rh)
            elif name != "off":
                self.obj = raster.TriUpscale(rw, rh, OUT_W, OUT_H)
                self.period = raster.upscale_jitter_period(rw, rh, OUT_W, OUT_H)
            if self.obj is not None:
                self.r.set_motion_output(True)
            self.index, self.cache = 0, {}

        def frame(self):
            """One frame of the chain: under the jitter contract when a pass follows."""
            s, r = self.scene, self.r
            if self.obj is None:
                r.render()
                return
            k = self.index % self.period
            self.index += 1
            if k not in self.cache:  # the period's jittered blocks are made once: the host keeps ahead of the device
                jx, jy = raster.taa_jitter(k, self.period)
                ubo = abi.TriGlobalUbo.from_buffer_copy(s.ubo)
                ubo.projection = (abi.C.c_float * 16)(*raster.taa_jitter_projection(self.proj, jx, jy, s.width, s.height).tolist())
                self.cache[k] = (jx, jy, ubo, raster.taa_jitter_projection(self.hist[1], jx, jy, s.width, s.height))
            jx, jy, ubo, prev_proj = self.cache[k]
            r.set_frame(ubo, s.clear)
            r.set_motion_history(self.hist[0], prev_proj, self.hist[2])
            r.render()
            if self.name == "taa_4k":
                self.obj.resolve(r, ALPHA)
            else:
                self.obj.resolve(r, (jx, jy), ALPHA)

        def window(self, frames):
            self.r.render_frame()  # switches and buffer growth happen outside the timed window
            self.frame()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(frames):
                self.frame()
            e1.record(stream)
            self.r.synchronize()
            return frames / (e0.elapsed_time(e1) * 1e-3)

        def pass_us(self, frames):
            self.frame()
            self.r.synchronize()
            t0 = self.obj.timing()
            self.r.set_timing(True)
            us = []
            for _ in range(frames):
                self.frame()
                self.r.synchronize()
                t1 = self.obj.timing()
                assert t1[1] == t0[1] + 1
                us.append(1e3 * (t1[0] - t0[0]))
                t0 = t1
            self.r.set_timing(False)
            return us

    todo = [("off", OUT_W, OUT_H)] + ([] if parent else list(CHAINS))
    chains = [Chain(*c) for c in todo]
    fps = {c.name: [] for c in chains}
    for c in chains:
        c.window(10)
    for _ in range(args.windows):
        for c in chains:
            fps[c.name].append(c.window(args.frames))
    for c in chains:
        entry = {"fps": stat(fps[c.name]), "render": [c.scene.width, c.scene.height]}
        if c.obj is not None:
            entry["pass_us"] = c.pass_us(args.frames)
            mask = c.obj.read()[2]
            entry["valid_fraction"] = float(((mask & 15) == 0).mean())
            entry["clamped_fraction"] = float(((mask & 32) != 0).mean())
            entry["no_sample_fraction"] = float(((mask & 64) != 0).mean())
            entry["jitter_period"] = c.period
            c.obj.close()
        c.r.close()
        out[c.name] = entry
    return out


def child(args, which):
    env = dict(os.environ)
    if which == "parent":
        env["TRI_RASTER_LIB"] = os.path.abspath(args.parent_lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--windows", str(args.windows),
                        "--frames", str(args.frames)], env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.exit(f"upscale_cost.py: the {which} child failed:\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def brief(t):
    return {"median": t["median"], "spread": t["spread"], "count": len(t["samples"])}


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
            print(f"upscale_cost.py: {which} child {len(runs[which])} of {args.rounds} done", file=sys.stderr, flush=True)

    def pooled(which, name):
        return stat([s for run in runs[which] for s in run[name]["fps"]["samples"]])

    result = {"frames_per_window": args.frames, "windows": args.windows, "rounds": args.rounds, "device": runs["tree"][0]["device"],
              "copy_bytes_per_s": COPY_BYTES_PER_S, "output": [OUT_W, OUT_H], "alpha": ALPHA,
              "bytes_per_output_pixel": BYTES_PER_OUTPUT_PIXEL, "bytes_per_render_pixel": BYTES_PER_RENDER_PIXEL,
              "taa_bytes_per_pixel": TAA_BYTES_PER_PIXEL}
    off = pooled("tree", "off")
    result["off"] = {"fps": off}
    if args.parent_lib:
        par = pooled("parent", "off")
        result["off"]["parent_fps"] = par
        result["off"]["tree_median_inside_parent_spread"] = par["spread"][0] <= off["median"] <= par["spread"][1]
    for name, rw, rh in CHAINS:
        us = stat([s for run in runs["tree"] for s in run[name]["pass_us"]])
        floor_us = 1e6 * floor_bytes(name, rw, rh) / COPY_BYTES_PER_S
        first = runs["tree"][0][name]
        result[name] = {
            "render": [rw, rh], "chain_fps": pooled("tree", name), "pass_us": brief(us),
            "traffic_bytes": floor_bytes(name, rw, rh), "traffic_floor_us": floor_us,
            "pass_fraction_of_copy_rate": floor_us / us["median"], "jitter_period": first["jitter_period"],
            "valid_fraction": statistics.median(run[name]["valid_fraction"] for run in runs["tree"]),
            "clamped_fraction": statistics.median(run[name]["clamped_fraction"] for run in runs["tree"]),
            "no_sample_fraction": statistics.median(run[name]["no_sample_fraction"] for run in runs["tree"]),
        }
    for name in ("up_1080p", "up_1440p"):
        result[name]["chain_fps_over_taa_4k"] = result[name]["chain_fps"]["median"] / result["taa_4k"]["chain_fps"]["median"]
    print(json.dumps(result, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
