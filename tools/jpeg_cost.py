#!/usr/bin/env python3
"""What Motion-JPEG recording costs on one GPU, and what the restart interval does to it.

Two parts, each in a fresh child process per repeat (the parent only collects):
  kernels   a rendered frame (C2's sphere at 1920x1080, C3's grid at 3840x2160) is captured from its device image with
            tri_recorder_capture_image, once per restart interval candidate: the device time of the four kernels
            (events around one capture at a time, as the slot protocol runs it), the stream's size, the bytes that
            cross the bus per frame (the size word, then the stream rounded up to 256) and the host time of one whole
            capture -> wait round. The YUV 4:4:4 recorder on the same frame is the comparison: 3 B/pixel copied.
  yuv444    with --parent-lib, a library built from the parent commit (tools/build_commit_variant.sh): the capture ring
            gained the variable-size product, so the Y4M recorder's capture -> wait -> release round behind a rendered
            frame (tri_recorder_create / capture / wait, which both libraries have) is timed on the host clock in
            children that alternate between the parent's library and this tree's; the tree's median must not exceed
            the slowest of the parent's own runs.
  engine    DrawFrames per second through TridentApp with 3 frames in flight: recording off, to .y4m and to .mkv (files
            under the system temp directory), windows alternating.
Medians with min-max over the repeats.

    python tools/jpeg_cost.py --out profiles/jpeg_cost.json [--parent-lib path/to/parent/libtri_raster.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = {"c2_1080p": ("c2", 1920, 1080), "c3_4k": ("c3", 3840, 2160)}


def candidates(width):
    row = (width + 15) // 16
    return [1, 2, 4, 5, 10, 20, 40, row]


def child_kernels(case, quality, rounds):
    import torch
    from trident_raster import abi, raster, scenes

    scene_name, w, h = CASES[case]
    s = scenes.scene_c2_sphere(w, h) if scene_name == "c2" else scenes.scene_c3_grid(w, h)
    out = {"width": w, "height": h, "quality": quality, "restart": {}}
    with raster.TriRaster(w, h, device=0) as r:
        scenes.load_scene(r, s)
        r.render_frame()
        img = r.output_image()

        def measure(rec, wait):
            for _ in range(3):
                rec.capture_image(0, img.device_ptr, img.pitch_bytes)
                n = wait(rec)
                rec.release(0)
            torch.cuda.synchronize()
            dev, host = [], []
            for _ in range(rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                rec.capture_image(0, img.device_ptr, img.pitch_bytes)  # the null stream, as the events
                e1.record()
                n = wait(rec)
                host.append((time.perf_counter() - t0) * 1e3)
                rec.release(0)
                torch.cuda.synchronize()
                dev.append(e0.elapsed_time(e1) * 1e3)
            return statistics.median(dev), statistics.median(host), n

        for restart in candidates(w):
            with raster.TriRecorder(w, h, 1, device=0, fmt=abi.TRI_RECORD_JPEG420, quality=quality, restart_mcus=restart) as rec:
                dev_us, host_ms, n = measure(rec, lambda rc: int(rc.wait_ex(0).size))
            out["restart"][str(restart)] = {"device_us": dev_us, "round_ms": host_ms, "stream_bytes": n,
                                            "copied_bytes": 4 + min((n + 255) & ~255, raster.jpeg_max_bytes(w, h, quality, restart)),
                                            "intervals": -(-(((w + 15) // 16) * ((h + 15) // 16)) // restart)}
        with raster.TriRecorder(w, h, 1, device=0) as rec:
            dev_us, host_ms, n = measure(rec, lambda rc: int(rc.wait(0).size))
        out["yuv444"] = {"device_us": dev_us, "round_ms": host_ms, "copied_bytes": n}
    print(json.dumps(out))


def child_yuv(case, rounds):
    """The Y4M recorder's round through the entry points the parent has too (this process's library)."""
    from trident_raster import raster, scenes

    scene_name, w, h = CASES[case]
    s = scenes.scene_c2_sphere(w, h) if scene_name == "c2" else scenes.scene_c3_grid(w, h)
    with raster.TriRaster(w, h, device=0) as r, raster.TriRecorder(w, h, 1, device=0) as rec:
        scenes.load_scene(r, s)
        r.render_frame()
        samples = []
        for k in range(rounds + 3):
            t0 = time.perf_counter()
            rec.capture(0, r)
            rec.wait_pointer(0)
            rec.release(0)
            if k >= 3:
                samples.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"round_ms": statistics.median(samples)}))


def child_engine(case, frames, quality):
    from record_cost import build_app, window_off

    scene_name, w, h = CASES[case]
    a, _ = build_app(scene_name, w, h, 3)
    a.set_recording_quality(quality)

    def window(path):
        a.finish_frame()
        t0 = time.perf_counter()
        assert a.set_recording(True, 1, w, h, path)[0]
        for _ in range(frames):
            a.draw_frame()
        assert a.set_recording(False)[0]
        dt = time.perf_counter() - t0
        size = os.path.getsize(path)
        os.remove(path)
        return frames / dt, size / frames

    out = {}
    with tempfile.TemporaryDirectory(prefix="jpeg_cost_") as tmp:
        window_off(a, 20)
        window(os.path.join(tmp, "w.mkv"))
        out["off_fps"] = window_off(a, frames * 3)
        out["mkv_fps"], out["mkv_bytes_per_frame"] = window(os.path.join(tmp, "a.mkv"))
        out["y4m_fps"], out["y4m_bytes_per_frame"] = window(os.path.join(tmp, "a.y4m"))
    a.close()
    print(json.dumps(out))


def run_child(args, lib=None):
    env = dict(os.environ)
    if lib:
        env["TRI_RASTER_LIB"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=600, env=env)
    if p.returncode != 0:
        sys.exit(f"child {args} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="c2_1080p,c3_4k")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libtri_raster.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs="*", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        kind, case = args.child[0], args.child[1]
        if kind == "kernels":
            child_kernels(case, args.quality, args.rounds)
        elif kind == "yuv":
            child_yuv(case, args.rounds)
        else:
            child_engine(case, args.frames, args.quality)
        return
    result = {"quality": args.quality, "repeats": args.repeats, "cases": {}}
    common = ["--quality", str(args.quality), "--rounds", str(args.rounds), "--frames", str(args.frames)]
    for case in args.cases.split(","):
        kernels = [run_child(common + ["--child", "kernels", case]) for _ in range(args.repeats)]
        entry = {"width": kernels[0]["width"], "height": kernels[0]["height"], "restart": {}}
        for key in kernels[0]["restart"]:
            rows = [k["restart"][key] for k in kernels]
            entry["restart"][key] = {"device_us": spread([r["device_us"] for r in rows]),
                                     "round_ms": spread([r["round_ms"] for r in rows]),
                                     "stream_bytes": rows[0]["stream_bytes"], "copied_bytes": rows[0]["copied_bytes"],
                                     "intervals": rows[0]["intervals"]}
        entry["yuv444"] = {"device_us": spread([k["yuv444"]["device_us"] for k in kernels]),
                           "round_ms": spread([k["yuv444"]["round_ms"] for k in kernels]),
                           "copied_bytes": kernels[0]["yuv444"]["copied_bytes"]}
        if args.parent_lib:
            runs = {"parent": [], "tree": []}
            for _ in range(args.repeats):  # alternating
                for which in ("parent", "tree"):
                    runs[which].append(run_child(common + ["--child", "yuv", case],
                                                 args.parent_lib if which == "parent" else None)["round_ms"])
            par, tree = spread(runs["parent"]), spread(runs["tree"])
            entry["yuv444_round_ms_ab"] = {"parent": par, "tree": tree,
                                           "tree_median_at_most_parent_max": tree["median"] <= par["max"]}
        if not args.skip_engine:
            engine = [run_child(common + ["--child", "engine", case]) for _ in range(args.repeats)]
            entry["engine"] = {k: spread([e[k] for e in engine]) for k in engine[0]}
        result["cases"][case] = entry
    print(json.dumps(result, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
