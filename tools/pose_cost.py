#!/usr/bin/env python3
"""What animating a scene costs, through the shim at 1920x1080: N instances (1, 64, 1024) of a skinned 24-bone
character, all playing a clip, with SetFramesInFlight(1) and (3), for
  (a) upload   matrices computed outside (precomputed here) and handed in for all entities with one call
               (trident_app_set_entities_bones), then uploaded: all there was before clip playback existed;
  (b) cpu      ECS::AnimationSystem evaluating every pose on the CPU, then the upload;
  (c) device   Renderer::SetDevicePoseEnabled: the system advances time, k_pose writes the palette on the device.
Reported per case: frames/s over a train of frames and host milliseconds per update + DrawFrame. And k_pose alone
through the C-ABI: microseconds per tri_pose_palette call from events around a train of calls on one stream.

    python tools/pose_cost.py --out profiles/pose_cost.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-renderer_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1920, 1080
BONES = 24


def character():
    """A 24-bone rig (a spine of 8 with two 8-bone limbs) from the tests' rig builder, with its two clips."""
    import anim_ref

    parents = [-1] + list(range(7)) + [3] + list(range(8, 15)) + [3] + list(range(16, 23))
    return anim_ref.make_rig("pose_cost_character", parents, 24)


def skinned_cube(scenes, np):
    v, i = scenes.cube_mesh()
    v = v.copy()
    v["bone_indices"][:, 0] = (np.arange(len(v)) * 5) % BONES
    v["bone_weights"][:] = 0.0
    v["bone_weights"][:, 0] = 1.0
    return v, i


def shim_case(app, anim_cases, scenes, np, rig, n, mode, inflight, frames):
    h, clips = anim_cases.cpu_asset(rig)
    a = app.TridentApp()
    a.set_frames_in_flight(inflight)
    a.set_camera("editor", (0.0, 0.0, 40.0))
    a.set_viewport(1, W, H)
    a.add_light("directional", direction=(-0.5, -1.0, -0.3), intensity=4.0)
    mesh = a.append_mesh(*skinned_cube(scenes, np))
    side = int(np.ceil(np.sqrt(n)))
    ents = [a.add_mesh_entity("none", mesh, position=(1.5 * (k % side - side / 2), 1.5 * (k // side - side / 2), 0.0))
            for k in range(n)]
    poses = [app.anim_evaluate(h, clips[1], 0.01 * k) for k in range(8)]
    handed = [np.stack([poses[(k + j) % 8] for j in range(n)]) for k in range(8)]  # per frame: [entities, bones, 16]
    if mode != "upload":
        for k, e in enumerate(ents):
            a.set_entity_animation(e, "test:" + rig.name, "test:" + rig.name, "slerp", time=0.37 * (k % 5), speed=1.0)
    a.set_device_pose(mode == "device")

    def frame(k):
        if mode == "upload":
            a.set_entities_bones(ents, handed[k % 8])
        else:
            a.update_animation(1.0 / 60.0)
        a.draw_frame()

    for k in range(6):
        frame(k)
    a.finish_frame()
    host = []
    t0 = time.perf_counter()
    for k in range(frames):
        s = time.perf_counter()
        frame(k)
        host.append(time.perf_counter() - s)
    a.finish_frame()
    wall = time.perf_counter() - t0
    uploads = a.bone_palette_uploads()
    a.close()
    return {"frames_per_s": frames / wall, "host_ms_per_frame": 1e3 * statistics.median(host), "palette_uploads": uploads}


def kernel_case(raster, anim_cases, torch, rig, n, calls):
    stream = torch.cuda.Stream()
    with raster.TriRaster(64, 64, device=0) as ctx, raster.TriAnimSet(0) as aset:
        sk, clips = anim_cases.device_asset(aset, rig)
        ctx.set_stream(stream.cuda_stream)
        inst = [(sk, clips[1], 0.013 * (k % 70), BONES * k) for k in range(n)]
        ctx.pose_palette(aset, inst)  # growth outside the train
        ctx.read_bone_palette(1)
        samples = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(calls):
                ctx.pose_palette(aset, inst)
            e1.record(stream)
            ctx.read_bone_palette(1)
            samples.append(e0.elapsed_time(e1) * 1e3 / calls)
        ctx.set_stream(None)
    return {"us_per_call": statistics.median(samples), "us_per_call_spread": [min(samples), max(samples)]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--counts", default="1,64,1024")
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("pose_cost.py measures on a GPU: none found")
    import anim_cases
    from trident_raster import app, raster, scenes

    raster.load_library()
    app.load_library()
    rig = character()
    result = {"device": torch.cuda.get_device_name(0), "width": W, "height": H, "bones": BONES, "frames": args.frames,
              "shim": {}, "k_pose": {}}
    for n in (int(c) for c in args.counts.split(",")):
        result["k_pose"][str(n)] = kernel_case(raster, anim_cases, torch, rig, n, 20)
        for inflight in (1, 3):
            for mode in ("upload", "cpu", "device"):
                result["shim"][f"n{n}_inflight{inflight}_{mode}"] = shim_case(app, anim_cases, scenes, np, rig, n, mode,
                                                                            inflight, args.frames)
    print(json.dumps(result, sort_keys=True))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
