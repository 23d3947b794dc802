#!/usr/bin/env python3
"""What the AI input tensor costs, on one GPU: the conversion kernel alone and tensors per second by every route.

Per case (C2's 50k-triangle sphere at 1920x1080, C3's 1M-triangle grid at 3840x2160):
  kernel         k_bgra_to_rgba_f32 alone, by device events around a train of tri_convert_rgba_f32 calls: time per
                 call and achieved bytes/s against the 20 B/pixel it must move (4 read + 16 written) and the HBM peak of
                 bench.py's roofline; k_bgra_to_yuv444 (7 B/pixel) the same way, for comparison on the same box; and
                 the dword-store path (an output that is only 4-B aligned);
  shim           tensors/s through the engine API with both throttles at 0: DrawFrame + TryAcquireRenderedFrame (into
                 a buffer the consumer reuses) each frame, at 1 and at 3 frames in flight: device conversion, pinned
                 copy, and the host copies that bring the tensor to the consumer. The tensor reaches the consumer one
                 frame (1 in flight) or three frames (3 in flight) after its DrawFrame, so each costs two host copies;
  shim_fenced    the same at 1 frame in flight with FinishFrame before the acquisition: the tensor of the frame just
                 drawn, taken straight from the pinned buffer (one host copy), the renderer not pipelined;
  device_only    tensors/s when the tensor stays on the GPU: tri_render + tri_framegrab_capture without
                 TRI_GRAB_HOST_COPY, three slots, the consumer waiting for each slot's conversion event;
  baseline       the route without any of it: DrawFrame + ReadViewportPixels (a fence and a blocking copy) + the host
                 conversion byte * (1 / 255) in float32 (numpy's vectorised loop, which is faster than the reference's
                 scalar one: the ratio reported is the conservative one).
Every step runs in a child process of its own under `timeout`; the first failing step ends the run.

    python tools/dataset_cost.py --out profiles/round8/dataset_cost.json
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0  # bench.py's roofline peak
CASES = {"c2_1080p": ("c2", 1920, 1080, 90), "c3_4k": ("c3", 3840, 2160, 30)}  # scene, extent, frames per window
STEP_SECONDS = {"kernel": 120, "shim1": 240, "shim3": 240, "shim_fenced": 240, "device_only": 240, "baseline": 240}


def _median(samples, scale=1.0):
    return {"median": statistics.median(samples) * scale, "spread": [min(samples) * scale, max(samples) * scale]}


def step_kernel(width, height, reps=50):
    import torch
    from trident_raster import raster

    px = width * height
    src = torch.randint(0, 256, (px * 4,), dtype=torch.uint8, device="cuda:0")
    f32 = torch.empty(px * 4 + 4, dtype=torch.float32, device="cuda:0")
    yuv = torch.empty(px * 3, dtype=torch.uint8, device="cuda:0")
    assert f32.data_ptr() % 16 == 0
    runs = {
        "rgba_f32": (lambda: raster.convert_rgba_f32(src.data_ptr(), width, height, width * 4, f32.data_ptr()), 20.0),
        "rgba_f32_dword_path": (lambda: raster.convert_rgba_f32(src.data_ptr(), width, height, width * 4,
                                                                f32.data_ptr() + 4), 20.0),
        "yuv444": (lambda: raster.convert_yuv444(src.data_ptr(), width, height, width * 4, yuv.data_ptr()), 7.0),
    }
    out = {}
    for name, (fn, bytes_per_pixel) in runs.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        samples = []
        for _ in range(3):  # three trains of `reps` calls between two events on the null stream
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples.append(e0.elapsed_time(e1) / reps)
        us = _median(samples, 1e3)
        gbs = bytes_per_pixel * px / (us["median"] * 1e-6) / 1e9
        out[name] = {"us": us["median"], "us_spread": us["spread"], "bytes_per_pixel": bytes_per_pixel,
                     "gb_per_s": gbs, "hbm_peak_frac": gbs / HBM_PEAK_GBS}
    out["rgba_f32_over_yuv444_bytes_per_s"] = out["rgba_f32"]["gb_per_s"] / out["yuv444"]["gb_per_s"]
    return out


def _windows(fn, repeats):
    fn(warm=True)
    return [fn(warm=False) for _ in range(repeats)]


def step_shim(scene, width, height, frames, inflight, repeats, fenced=False):
    import numpy as np
    import record_cost

    a, _ = record_cost.build_app(scene, width, height, inflight)
    assert a.set_ai_readback(True, 0, 0)
    buf = np.zeros(width * height * 4, np.float32)  # the consumer's buffer, reused (touched once: no page faults later)

    def window(warm):
        n = 6 if warm else frames
        a.finish_frame()
        while a.acquire_frame(buf) is not None:
            pass
        got = 0
        t0 = time.perf_counter()
        for _ in range(n):
            a.draw_frame()
            if fenced:
                a.finish_frame()
            got += a.acquire_frame(buf) is not None
        a.finish_frame()
        got += a.acquire_frame(buf) is not None
        dt = time.perf_counter() - t0
        assert got >= n - inflight, (got, n)  # (a frame resolved between two acquisitions replaces the one before)
        return got / dt

    try:
        v = _windows(window, repeats)
    finally:
        a.close()
    m = _median(v)
    return {"tensors_per_s": m["median"], "tensors_per_s_spread": m["spread"], "frames_per_window": frames}


def step_baseline(scene, width, height, frames, repeats):
    import numpy as np
    import record_cost

    a, _ = record_cost.build_app(scene, width, height, 3)
    inv = np.float32(1) / np.float32(255)

    def window(warm):
        n = 2 if warm else frames
        a.finish_frame()
        t0 = time.perf_counter()
        for _ in range(n):
            a.draw_frame()
            rgba, _ = a.read_pixels(1, width, height, depth=False)
            tensor = rgba.astype(np.float32) * inv
            assert tensor.shape == (height, width, 4)
        return n / (time.perf_counter() - t0)

    try:
        v = _windows(window, repeats)
    finally:
        a.close()
    m = _median(v)
    return {"tensors_per_s": m["median"], "tensors_per_s_spread": m["spread"], "frames_per_window": frames}


def step_device_only(scene, width, height, frames, repeats):
    from trident_raster import raster, scenes

    s = scenes.scene_c2_sphere(width, height) if scene == "c2" else scenes.scene_c3_grid(width, height)
    slots = 3
    with raster.TriRaster(width, height) as r, raster.FrameGrab(width, height, slots) as grab:
        scenes.load_scene(r, s)

        def window(warm):
            n = 6 if warm else frames
            r.synchronize()
            t0 = time.perf_counter()
            for k in range(n):
                if k >= slots:  # the consumer takes the oldest tensor (its conversion event) and hands the slot back
                    assert grab.wait_pointers(k % slots, host=False)[1]
                    grab.release(k % slots)
                r.render()
                grab.capture(k % slots, r)
            for k in range(max(n - slots, 0), n):
                assert grab.wait_pointers(k % slots, host=False)[1]
                grab.release(k % slots)
            r.synchronize()
            return n / (time.perf_counter() - t0)

        v = _windows(window, repeats)
    m = _median(v)
    return {"tensors_per_s": m["median"], "tensors_per_s_spread": m["spread"], "frames_per_window": frames}


def run_step(step, case, repeats):
    scene, w, h, frames = CASES[case]
    from trident_raster import app, raster

    raster.load_library()
    app.load_library()
    if step == "kernel":
        return step_kernel(w, h)
    if step in ("shim1", "shim3"):
        return step_shim(scene, w, h, frames, 1 if step == "shim1" else 3, repeats)
    if step == "shim_fenced":
        return step_shim(scene, w, h, frames, 1, repeats, fenced=True)
    if step == "device_only":
        return step_device_only(scene, w, h, frames, repeats)
    if step == "baseline":
        return step_baseline(scene, w, h, max(frames // 6, 3), repeats)
    raise SystemExit("unknown step " + step)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="c2_1080p,c3_4k")
    ap.add_argument("--steps", default="kernel,shim1,shim3,shim_fenced,device_only,baseline")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)  # a child: one step of one case, JSON on stdout
    ap.add_argument("--case", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    import torch

    if args.step:
        if not torch.cuda.is_available():
            sys.exit("dataset_cost.py measures on a GPU: none found")
        print("RESULT " + json.dumps(run_step(args.step, args.case, args.repeats), sort_keys=True))
        return
    result = {"hbm_peak_gb_per_s": HBM_PEAK_GBS, "cases": {}}
    for case in args.cases.split(","):
        _, w, h, _ = CASES[case]
        entry = {"width": w, "height": h, "tensor_bytes": 16 * w * h}
        result["cases"][case] = entry
        for step in args.steps.split(","):
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--case", case, "--repeats", str(args.repeats)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not lines:  # the first failure ends the run: nothing more starts on the GPU
                sys.exit(f"dataset_cost.py: step {step} of {case} failed (exit status {p.returncode})")
            entry[step] = json.loads(lines[-1][len("RESULT "):])
            print(f"{case} {step}: {lines[-1][len('RESULT '):]}", flush=True)
        base = entry.get("baseline", {}).get("tensors_per_s")
        if base:
            entry["ratio_over_baseline"] = {k: entry[k]["tensors_per_s"] / base for k in ("shim1", "shim3", "shim_fenced", "device_only")
                                            if k in entry}
    print(json.dumps(result, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
