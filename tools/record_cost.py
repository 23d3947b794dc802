#!/usr/bin/env python3
"""What viewport recording costs, through the engine API (TridentApp, 3 frames in flight), on one GPU.

Per case (C2's 50k-triangle sphere at 1920x1080, C3's 1M-triangle grid at 3840x2160) it reports DrawFrames per second
  (a) off        recording off;
  (b) record     recording on, to a .y4m file under the system temp directory (device conversion, pinned copy,
                 SubmitPlanes at each frame's fence);
  (c) readback   the route without it: read_pixels every frame (fence + blocking copy of 4 B/pixel) and the host
                 VideoEncoder::SubmitFrame (fp64 conversion on one CPU core), to a file in the same directory;
and the parts of (b) on their own, so that it is visible which one bounds it:
  kernel_us      k_bgra_to_yuv444 alone (device events around a train of tri_convert_yuv444 calls, per call);
  d2h_ms         one frame's 3 B/pixel from device to pinned host memory (device events);
  write_ms       one FRAME record's bytes written to a file in the temp directory (host clock, flushed).
The windows alternate between the cases and repeat; the median is reported with the spread. A recorded window is
limited in frames, not in time: every 4K frame adds 24.9 MB to the file.

    python tools/record_cost.py --out profiles/round7/record_cost.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-renderer_amd", "python"))

CASES = {"c2_1080p": ("c2", 1920, 1080, 120), "c3_4k": ("c3", 3840, 2160, 36)}  # scene, extent, frames per window


def build_app(scene_name, width, height, inflight):
    from trident_raster import app, scenes

    a = app.TridentApp()
    a.set_assets_dir(scenes.ASSETS_DIR)
    a.set_frames_in_flight(inflight)
    if scene_name == "c2":
        s = scenes.scene_c2_sphere(width, height)
        mi = a.append_mesh(s.vertices, s.indices, base_color=(0.9, 0.75, 0.6, 1.0), metallic=0.3, roughness=0.45)
        a.add_mesh_entity("none", mi)
        rng = scenes.PCG32(0x5EED)
        a.add_light("point", position=(4.0, 3.0, 5.0), color=tuple(0.6 + 0.4 * rng.uniform(3)), intensity=6.0, range=15.0)
        a.add_light("point", position=(-4.0, -2.0, 4.0), color=tuple(0.6 + 0.4 * rng.uniform(3)), intensity=4.0, range=15.0)
        a.set_camera("editor", (0.0, 0.0, 9.0), (0.0, 0.0, 0.0), fov=60.0, near=0.1, far=1000.0)
    else:
        s = scenes.scene_c3_grid(width, height)
        mi = a.append_mesh(s.vertices, s.indices, base_color=(1.0, 1.0, 1.0, 1.0), metallic=0.1, roughness=0.6)
        a.add_mesh_entity("none", mi)
        a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=3.0)
        for k, (px, py) in enumerate([(-3.0, 1.5), (3.0, 1.5), (-3.0, -1.5), (3.0, -1.5)]):
            a.add_light("point", position=(px, py, -2.5), color=(1.0, 0.9 - 0.1 * k, 0.7 + 0.1 * k),
                        intensity=3.0 + k, range=8.0)
        a.set_camera("editor", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), fov=60.0, near=0.1, far=1000.0)
    a.set_viewport(1, width, height)
    return a, s.triangles


def window_off(a, frames):
    a.finish_frame()
    t0 = time.perf_counter()
    for _ in range(frames):
        a.draw_frame()
    a.finish_frame()
    return frames / (time.perf_counter() - t0)


def window_record(a, frames, width, height, path):
    a.finish_frame()
    t0 = time.perf_counter()
    ok, extent = a.set_recording(True, 1, width, height, path)
    assert ok and extent == (width, height), (ok, extent)
    for _ in range(frames):
        a.draw_frame()
    assert a.set_recording(False)[0]  # finishes the frames in flight and closes the file: part of the cost
    dt = time.perf_counter() - t0
    assert a.recording_state() == (False, frames)
    assert os.path.getsize(path) > frames * 3 * width * height
    os.remove(path)
    return frames / dt


def window_readback(a, frames, width, height, path):
    from trident_raster import app

    a.finish_frame()
    enc = app.VideoEncoder()
    t0 = time.perf_counter()
    assert enc.begin(path, width, height, 1)
    for _ in range(frames):
        a.draw_frame()
        rgba, _ = a.read_pixels(1, width, height, depth=False)
        assert enc.submit_rgba(rgba, width, height)
    assert enc.end()
    dt = time.perf_counter() - t0
    enc.close()
    os.remove(path)
    return frames / dt


def parts(width, height, tmpdir, reps=50):
    """The conversion kernel, the pinned copy and the file write of one frame, each on its own."""
    import torch
    from trident_raster import raster

    px = width * height
    src = torch.randint(0, 256, (px * 4,), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(px * 3, dtype=torch.uint8, device="cuda:0")
    host = torch.empty(px * 3, dtype=torch.uint8).pin_memory()
    convert = lambda: raster.convert_yuv444(src.data_ptr(), width, height, width * 4, dst.data_ptr())  # noqa: E731
    out = {}
    for name, fn in (("kernel_us", convert), ("d2h_ms", lambda: host.copy_(dst, non_blocking=True))):
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
        out[name] = statistics.median(samples) * (1e3 if name.endswith("_us") else 1.0)
        out[name + "_spread"] = [min(samples) * (1e3 if name.endswith("_us") else 1.0),
                                 max(samples) * (1e3 if name.endswith("_us") else 1.0)]
    out["kernel_gb_per_s"] = 7.0 * px / (out["kernel_us"] * 1e-6) / 1e9  # 4 B read + 3 B written per pixel
    out["d2h_gb_per_s"] = 3.0 * px / (out["d2h_ms"] * 1e-3) / 1e9
    payload = host.numpy().tobytes()
    path = os.path.join(tmpdir, "write_probe.y4m")
    samples = []
    for _ in range(3):
        t0 = time.perf_counter()
        with open(path, "wb") as f:
            for _ in range(8):
                f.write(b"FRAME\n")
                f.write(payload)
            f.flush()
        samples.append((time.perf_counter() - t0) / 8 * 1e3)
        os.remove(path)
    out["write_ms"] = statistics.median(samples)
    out["write_ms_spread"] = [min(samples), max(samples)]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="c2_1080p,c3_4k")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--inflight", type=int, default=3)
    ap.add_argument("--readback-frames", type=int, default=6, help="frames per window of case (c): seconds each at 4K")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("record_cost.py measures on a GPU: none found")
    from trident_raster import app, raster

    raster.load_library()
    app.load_library()
    result = {"frames_in_flight": args.inflight, "device": torch.cuda.get_device_name(0), "cases": {}}
    with tempfile.TemporaryDirectory(prefix="record_cost_") as tmp:
        for case in args.cases.split(","):
            scene, w, h, frames = CASES[case]
            a, tris = build_app(scene, w, h, args.inflight)
            try:
                rec_path, rb_path = os.path.join(tmp, "rec.y4m"), os.path.join(tmp, "readback.y4m")
                window_off(a, 30)  # warm-up of every path the windows use
                window_record(a, 6, w, h, rec_path)
                window_readback(a, 2, w, h, rb_path)
                fps = {"off": [], "record": [], "readback": []}
                for _ in range(args.repeats):  # alternating windows
                    fps["off"].append(window_off(a, frames * 4))
                    fps["record"].append(window_record(a, frames, w, h, rec_path))
                    fps["readback"].append(window_readback(a, args.readback_frames, w, h, rb_path))
                entry = {"scene": scene, "width": w, "height": h, "triangles": tris, "frames_per_window":
                         {"off": frames * 4, "record": frames, "readback": args.readback_frames},
                         "frame_bytes_yuv": 3 * w * h}
                for k, v in fps.items():
                    entry[k + "_fps"] = statistics.median(v)
                    entry[k + "_fps_spread"] = [min(v), max(v)]
                    entry[k + "_ms_per_frame"] = 1e3 / statistics.median(v)
            finally:
                a.close()
            entry["parts"] = parts(w, h, tmp)
            result["cases"][case] = entry
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
