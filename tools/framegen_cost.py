#!/usr/bin/env python3
"""What the frame generator costs, on one GPU.

  network   milliseconds per inference at 256x256 (the trainer's default) and at 1920x1080, by the generator's own
            device events around its 20 launches (tri_framegen_last_ms): the median of three windows of jobs and
            their spread; the same as a fraction of the float32 matrix peak (157 TFLOP/s) with the network's FLOPs
            counted layer by layer (2 x taps x Cin x Cout per output pixel of each layer); and torch eager float32 of
            the same network on the same GPU, by torch events, next to it;
  shim      frames/s of the C2 scene at 1920x1080 through the engine API (3 frames in flight) with the generator running
            with both throttles at 0 and at the reference's 66 ms, against the same scene with the AI readback on at
            the same throttles but no model (what the generator itself adds) and with neither;
  loop      tensors/s of the whole loop (frame -> tensor -> network -> blend frame) on the device, against the way
            without the generator: TryAcquireRenderedFrame, the network in torch on the GPU, SubmitAiOutput.
Every step runs in a child process of its own under `timeout`; the first failing step ends the run. The weights are
seeded random numbers in the checkpoint's shapes: the cost does not depend on their values.

    python tools/framegen_cost.py --out profiles/framegen_cost.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import framegen_ref  # noqa: E402  (the network restated once, for the tests and for this tool)

F32_MATRIX_PEAK_TFLOPS = 157.0
EXTENTS = {"256x256": (256, 256), "1920x1080": (1920, 1080)}
STEP_SECONDS = {"network": 240, "shim": 300, "loop": 300}


def _median(samples, scale=1.0):
    return {"median": statistics.median(samples) * scale, "spread": [min(samples) * scale, max(samples) * scale]}


def make_state(cin, seed=7):
    return {k: v for k, v in framegen_ref.make_state(cin, seed).items() if v.is_floating_point()}


def container(cin=4):
    import export_frame_generator

    return export_frame_generator.container_from_state(make_state(cin))


def step_network(jobs=10):
    import torch
    from trident_raster import raster

    blob = container(4)
    state = {k: v.cuda() for k, v in make_state(4).items()}
    flops = framegen_ref.flops_per_pixel(4)
    out = {"flops_per_pixel": flops}
    for name, (w, h) in EXTENTS.items():
        x = torch.rand((h, w, 4), device="cuda")
        with raster.FrameGenerator(blob, w, h) as gen:
            def one():
                gen.submit(x.data_ptr())
                gen.wait()
                return gen.last_ms()

            for _ in range(3):
                one()
            windows = [statistics.mean(one() for _ in range(jobs)) for _ in range(3)]
        ms = _median(windows)
        tf = flops * w * h / (ms["median"] * 1e-3) / 1e12
        xn = x.permute(2, 0, 1)[None].contiguous()
        with torch.no_grad():
            for _ in range(3):
                framegen_ref.forward_nchw(state, xn)
            torch.cuda.synchronize()
            eager = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(jobs):
                    framegen_ref.forward_nchw(state, xn)
                e1.record()
                torch.cuda.synchronize()
                eager.append(e0.elapsed_time(e1) / jobs)
        em = _median(eager)
        out[name] = {"ms": ms["median"], "ms_spread": ms["spread"], "tflops": tf, "f32_matrix_peak_frac": tf / F32_MATRIX_PEAK_TFLOPS,
                     "torch_eager_ms": em["median"], "torch_eager_ms_spread": em["spread"],
                     "torch_eager_over_generator": em["median"] / ms["median"]}
    return out


def _model_file(cin=4):
    f = tempfile.NamedTemporaryFile(suffix=".trifgen", delete=False)
    f.write(container(cin))
    f.close()
    return f.name


def step_shim(frames=90, width=1920, height=1080):
    import record_cost

    path = _model_file()
    out = {"width": width, "height": height, "frames_per_window": frames}
    try:
        for name, model, throttle in (("no_readback", False, None), ("readback_only_0ms", False, 0), ("throttle_0ms", True, 0),
                                      ("readback_only_66ms", False, 66), ("throttle_66ms", True, 66)):
            a, _ = record_cost.build_app("c2", width, height, 3)
            if model:
                a.load_ai_model(path)
            if throttle is not None:
                assert a.set_ai_readback(True, throttle, throttle)

            def window(n):
                a.finish_frame()
                t0 = time.perf_counter()
                for _ in range(n):
                    a.draw_frame()
                a.finish_frame()
                return n / (time.perf_counter() - t0)

            try:
                window(10)
                fps = _median([window(frames) for _ in range(3)])
                stats = a.ai_debug_stats()
                assert a.finish_ai_inference(20000)
            finally:
                a.close()
            out[name] = {"frames_per_s": fps["median"], "frames_per_s_spread": fps["spread"],
                         "completed_inferences": stats["completed_inference_count"],
                         "average_inference_ms": stats["average_inference_ms"]}
        for name in ("throttle_0ms", "throttle_66ms"):
            out[name]["over_readback_only"] = out[name]["frames_per_s"] / out[name.replace("throttle", "readback_only")]["frames_per_s"]
            out[name]["over_no_readback"] = out[name]["frames_per_s"] / out["no_readback"]["frames_per_s"]
    finally:
        os.unlink(path)
    return out


def step_loop(frames=30, width=1920, height=1080):
    import numpy as np
    import torch
    import record_cost

    path = _model_file()
    out = {"width": width, "height": height, "frames_per_window": frames}
    try:
        # on the device: every frame is fenced and its inference finished, so each frame yields one blend frame
        a, _ = record_cost.build_app("c2", width, height, 1)
        a.load_ai_model(path)
        assert a.set_ai_readback(True, 0, 0)

        def device_window(n):
            a.finish_frame()
            assert a.finish_ai_inference(20000)
            before = a.ai_debug_stats()["completed_inference_count"]
            t0 = time.perf_counter()
            for _ in range(n):
                a.draw_frame()
                a.finish_frame()
                assert a.finish_ai_inference(20000)
            dt = time.perf_counter() - t0
            done = a.ai_debug_stats()["completed_inference_count"] - before
            assert done >= n - 1, (done, n)
            return done / dt

        try:
            device_window(3)
            dev = _median([device_window(frames) for _ in range(3)])
        finally:
            a.close()
        # without the generator: the tensor to the host, the network in torch on the GPU, the output back through the host
        state = {k: v.cuda() for k, v in make_state(4).items()}
        a, _ = record_cost.build_app("c2", width, height, 1)
        assert a.set_ai_readback(True, 0, 0)
        buf = np.zeros(width * height * 4, np.float32)

        def manual_window(n):
            a.finish_frame()
            got = 0
            t0 = time.perf_counter()
            for _ in range(n):
                a.draw_frame()
                a.finish_frame()
                t = a.acquire_frame(buf)
                if t is None:
                    continue
                with torch.no_grad():
                    x = torch.from_numpy(t).cuda().permute(2, 0, 1)[None]
                    y = framegen_ref.forward_nchw(state, x)[0].permute(1, 2, 0).contiguous().cpu().numpy()
                assert a.submit_ai_output(y, (1, height, width, 3))
                got += 1
            dt = time.perf_counter() - t0
            assert got >= n - 1, (got, n)
            return got / dt

        try:
            manual_window(3)
            man = _median([manual_window(frames) for _ in range(3)])
        finally:
            a.close()
    finally:
        os.unlink(path)
    out["device"] = {"tensors_per_s": dev["median"], "tensors_per_s_spread": dev["spread"]}
    out["manual_torch"] = {"tensors_per_s": man["median"], "tensors_per_s_spread": man["spread"]}
    out["device_over_manual"] = dev["median"] / man["median"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", default="network,shim,loop")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)  # a child: one step, JSON on stdout
    args = ap.parse_args()
    if args.step:
        import torch
        from trident_raster import app, raster

        if not torch.cuda.is_available():
            sys.exit("framegen_cost.py measures on a GPU: none found")
        torch.cuda.init()
        raster.load_library()
        app.load_library()
        fn = {"network": step_network, "shim": step_shim, "loop": step_loop}[args.step]
        print("RESULT " + json.dumps(fn(), sort_keys=True))
        return
    result = {"f32_matrix_peak_tflops": F32_MATRIX_PEAK_TFLOPS}
    for step in args.steps.split(","):
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:  # the first failure ends the run: nothing more starts on the GPU
            sys.exit(f"framegen_cost.py: step {step} failed (exit status {p.returncode})")
        result[step] = json.loads(lines[-1][len("RESULT "):])
        print(f"{step}: {lines[-1][len('RESULT '):]}", flush=True)
    print(json.dumps(result, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
