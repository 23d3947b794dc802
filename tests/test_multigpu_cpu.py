"""N > 1 path on the CPU: world-size-2 (and 4) gloo process groups run bench.py's band partition,
band gather / all-gather and max-over-ranks timing, with and without cluster culling (a restatement
of k_vertex's cluster test drops the culled clusters' triangles from a band's render). Each rank renders its row band with the oracle (the
CPU stand-in for its GPU's k_raster band), and the gathered frame must equal a full-frame render.
Sort-first bands are exact: a pixel depends only on the triangles covering it.
"""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


CLUSTER_PRIMS = 512  # raster_common.h TRI_CLUSTER_PRIMS


def cluster_visible(scene, draw, lo, hi, y0, y1):
    """Restatement of k_vertex's cluster_visible (vertex_stage.hip): the object-space box through
    (P V) M; a box wholly in front of the eye whose image misses rows [y0, y1) or the frame's columns (2 px
    margin), or lies before z = 0 or beyond z = w, has no fragment in the band."""
    if (lo > hi).any():
        return False
    if draw.pc.bone_count > 0:
        return True
    u = scene.ubo
    view = np.array(u.view, np.float32).reshape(4, 4).T
    proj = np.array(u.projection, np.float32).reshape(4, 4).T
    model = np.array(draw.pc.model, np.float32).reshape(4, 4).T
    m = (proj @ view) @ model
    corners = np.array([[hi[0] if k & 1 else lo[0], hi[1] if k & 2 else lo[1], hi[2] if k & 4 else lo[2], 1.0]
                        for k in range(8)], np.float32)
    c = corners @ m.T
    if not (c[:, 3] > 1e-4).all():
        return True
    ndc = c[:, :3] / c[:, 3:4]
    hw, hh = scene.width / 2.0, scene.height / 2.0
    wx, wy = ndc[:, 0] * hw + hw, ndc[:, 1] * hh + hh
    return not (wy.max() < y0 - 2 or wy.min() > y1 + 2 or wx.max() < -2 or wx.min() > scene.width + 2 or
                ndc[:, 2].max() < 0 or ndc[:, 2].min() > 1)


def cull_clusters(scene, y0, y1):
    """The scene with every triangle of a cluster culled for rows [y0, y1) made degenerate (zero area:
    no fragment, primitive order unchanged); returns it and the number of culled clusters."""
    import copy

    s = copy.copy(scene)
    idx = scene.indices.copy()
    culled = 0
    for d in scene.draws:
        m = scene.meshes[d.mesh_index]
        f, n, bv = int(m["first_index"]), int(m["index_count"]), int(m["base_vertex"])
        assert sum(1 for e in scene.draws if e.mesh_index == d.mesh_index) == 1, "one draw per mesh"
        tris = idx[f:f + n - n % 3].reshape(-1, 3)
        for c0 in range(0, len(tris), CLUSTER_PRIMS):
            t = tris[c0:c0 + CLUSTER_PRIMS].astype(np.int64) + bv
            ok = t[(t >= 0) & (t < len(scene.vertices))]
            pos = scene.vertices["position"][ok].astype(np.float32)
            lo = pos.min(0) if len(pos) else np.full(3, np.inf, np.float32)
            hi = pos.max(0) if len(pos) else np.full(3, -np.inf, np.float32)
            if not cluster_visible(scene, d, lo, hi, y0, y1):
                culled += 1
                tris[c0:c0 + CLUSTER_PRIMS] = tris[c0:c0 + CLUSTER_PRIMS, :1]
        idx[f:f + len(tris) * 3] = tris.reshape(-1)
    s.indices = idx
    return s, culled


def _worker(rank, world, port, scene_name, out_dir, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "3d-renderer_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    import torch.distributed as dist

    import bench
    import oracle_py
    import scene_cases as sc

    dist.init_process_group("gloo", rank=rank, world_size=world)
    scene = getattr(sc, scene_name)()
    W, H = scene.width, scene.height
    y0, y1 = bench.band_rows(H, world, rank)
    if mode.endswith("+cull"):  # the band renders only the triangles of its visible clusters
        mode = mode[:-5]
        scene, culled = cull_clusters(scene, y0, y1)
        np.save(os.path.join(out_dir, f"culled{rank}.npy"), np.array([culled]))
    col, dep, _ = oracle_py.render(scene, band=(y0, y1), threads=2)
    band = torch.from_numpy(np.ascontiguousarray(col).view(np.int32).reshape(-1).copy())
    dband = torch.from_numpy(np.ascontiguousarray(dep).view(np.int32).reshape(-1).copy())
    frame = torch.empty(H * W, dtype=torch.int32)
    dframe = torch.empty(H * W, dtype=torch.int32)
    out = bench.gather_bands(frame, band, world, mode=mode, rank=rank)
    dout = bench.gather_bands(dframe, dband, world, mode=mode, rank=rank)
    slowest = bench.max_over_ranks(float(rank + 1), torch.device("cpu"), True)
    if out is not None:  # gather mode: only the display rank (0) holds the frame
        np.save(os.path.join(out_dir, f"frame{rank}.npy"), out.numpy())
        np.save(os.path.join(out_dir, f"depth{rank}.npy"), dout.numpy())
    np.save(os.path.join(out_dir, f"slowest{rank}.npy"), np.array([slowest]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,scene_name,mode", [(2, "c1_cube", "gather"), (4, "textured_grid", "gather"),
                                                   (2, "textured_grid", "allgather"),
                                                   (2, "textured_grid", "gather+cull"),
                                                   (4, "textured_grid", "gather+cull")])
def test_row_band_assembly_equals_full_frame(world, scene_name, mode, oracle, tmp_path):
    import torch.multiprocessing as mp

    import scene_cases as sc

    port = _free_port()
    mp.start_processes(_worker, args=(world, port, scene_name, str(tmp_path), mode), nprocs=world, join=True,
                       start_method="spawn")
    scene = getattr(sc, scene_name)()
    col, dep, _ = oracle.render(scene, threads=4)
    if mode.endswith("+cull"):  # the partition with cluster culling: some band culled something
        mode = mode[:-5]
        assert sum(int(np.load(tmp_path / f"culled{r}.npy")[0]) for r in range(world)) > 0
    full = np.ascontiguousarray(col).view(np.int32).reshape(-1)
    dfull = np.ascontiguousarray(dep).view(np.int32).reshape(-1)
    for r in range(world):
        if mode == "allgather" or r == 0:
            assert np.array_equal(np.load(tmp_path / f"frame{r}.npy"), full), f"rank {r} colour"
            assert np.array_equal(np.load(tmp_path / f"depth{r}.npy"), dfull), f"rank {r} depth"
        else:
            assert not (tmp_path / f"frame{r}.npy").exists()
        assert float(np.load(tmp_path / f"slowest{r}.npy")[0]) == float(world)


def _ring_worker(rank, world, port, out_dir, mode):
    """bench.GatherRing over gloo: 5 frames through the double buffer, each band stamped with
    (frame, rank); every assembled frame must hold exactly that frame's bands."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    import bench

    dist.init_process_group("gloo", rank=rank, world_size=world)
    rows, W = 3, 5
    ring = bench.GatherRing(world, rows * W, world * rows * W, lambda n: torch.zeros(n, dtype=torch.int32), mode=mode,
                            rank=rank)
    assembled = []
    for k in range(5):
        band = ring.acquire()
        band.fill_(1000 * k + rank)  # the "render" of frame k into this rank's band
        ring.publish()
        if k % 2 == 1:  # read back every other frame only after its gather completed
            ring.drain()
            assembled.append((k, ring.frame.clone().numpy()))
    ring.drain()
    assembled.append((4, ring.frame.clone().numpy()))
    for k, fr in assembled:
        if mode == "allgather" or rank == 0:
            np.save(os.path.join(out_dir, f"ring{rank}_{k}.npy"), fr)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["gather", "allgather"])
def test_gather_ring_double_buffer(mode):
    import torch.multiprocessing as mp

    import tempfile

    world = 2
    with tempfile.TemporaryDirectory() as d:
        mp.start_processes(_ring_worker, args=(world, _free_port(), d, mode), nprocs=world, join=True,
                           start_method="spawn")
        for r in (range(world) if mode == "allgather" else [0]):
            for k in (1, 3, 4):
                fr = np.load(os.path.join(d, f"ring{r}_{k}.npy")).reshape(world, -1)
                for src in range(world):
                    assert (fr[src] == 1000 * k + src).all(), (r, k, src)


def test_band_rows_partition():
    sys.path.insert(0, ROOT)
    import bench

    for H, N in [(2160, 1), (2160, 2), (2160, 4), (2160, 8), (1080, 8), (480, 2)]:
        bands = [bench.band_rows(H, N, r) for r in range(N)]
        assert bands[0][0] == 0 and bands[-1][1] == H
        assert all(bands[i][1] == bands[i + 1][0] for i in range(N - 1))
        assert len({b[1] - b[0] for b in bands}) == 1
    with pytest.raises(ValueError):
        bench.band_rows(1081, 2, 0)


def test_band_split_partition():
    """bench.band_split: contiguous bands covering [0, H) top to bottom; equal by default (within one row,
    any height); with display_rows, rank 0 takes exactly that many and the others within one row of each
    other."""
    sys.path.insert(0, ROOT)
    import bench

    for H, N, d in [(2160, 1, None), (2160, 2, None), (2161, 3, None), (2160, 8, None), (2160, 2, 1400),
                    (2160, 8, 540), (1080, 8, 300), (480, 4, 121)]:
        bands = bench.band_split(H, N, d)
        assert len(bands) == N and bands[0][0] == 0 and bands[-1][1] == H
        assert all(bands[i][1] == bands[i + 1][0] for i in range(N - 1))
        sizes = [b - a for a, b in bands]
        rest = sizes if d is None else sizes[1:]
        if rest:
            assert max(rest) - min(rest) <= 1
        if d is not None and N > 1:
            assert sizes[0] == d
    with pytest.raises(ValueError):
        bench.band_split(100, 4, 98)
    assert bench.split_candidates(2160, 8)[0] == (270, 2)
    assert all(2160 - d >= 7 * 32 for d, _ in bench.split_candidates(2160, 8, inflights=(2, 3)))
    assert bench.split_candidates(2160, 2)[-1][0] <= 2160 - 32
    assert {k for _, k in bench.split_candidates(2160, 4, inflights=(2, 3))} == {2, 3}
    # a small frame over a large world keeps the equal split (no empty candidate list)
    assert bench.split_candidates(240, 8) == [(30, 2)]
    # an assemble-only display (0 rows: the native exchange's display renders nothing) is a candidate when asked for
    # and the other ranks keep at least one bin row each; never at N = 2 (one sender would render the whole frame)
    bands = bench.band_split(2160, 8, 0)
    assert bands[0] == (0, 0) and [b - a for a, b in bands[1:]] == [309] * 4 + [308] * 3
    assert 0 not in [d for d, _ in bench.split_candidates(2160, 8)]
    assert [d for d, _ in bench.split_candidates(2160, 8, inflights=(2, 3), assemble_only=True)].count(0) == 2
    assert 0 not in [d for d, _ in bench.split_candidates(2160, 2, assemble_only=True)]
    assert 0 not in [d for d, _ in bench.split_candidates(200, 8, assemble_only=True)]
    with pytest.raises(ValueError):
        bench.band_split(2160, 8, -1)
    # explicit band sizes, and the rebalancing step's re-cut: rows move from the slow bands to the fast ones, the
    # display band is kept, the rows still cover the frame, equal times change nothing
    assert bench.band_split(100, 3, (0, 60, 40)) == [(0, 0), (0, 60), (60, 100)]
    for bad in [(0, 60, 39), (10, 90), (0, 100, 0)]:
        with pytest.raises(ValueError):
            bench.band_split(100, 3, bad)
    new = bench.rebalance_sizes(bands, [0.0, 26.7, 26.5, 26.4, 26.4, 26.6, 26.9, 27.4])
    assert new[0] == 0 and sum(new) == 2160 and new[7] < 308 and new[4] > 309 and min(new[1:]) >= 32
    assert bench.band_split(2160, 8, tuple(new))[-1] == (2160 - new[7], 2160)
    b67 = bench.band_split(2160, 8, 67)
    assert bench.rebalance_sizes(b67, [30.0] + [26.0] * 7) == [b - a for a, b in b67]
    tiny = bench.rebalance_sizes(bench.band_split(300, 8, 0), [1.0] * 7 + [100.0])  # a very slow band keeps min_rows
    assert tiny[7] == 32 and sum(tiny) == 300 and max(tiny[1:7]) - min(tiny[1:7]) <= 1


def _uneven_worker(rank, world, port, scene_name, out_dir, display_rows, ring):
    """Uneven sort-first bands (a larger display band) rendered by the oracle per rank and assembled by
    bench.gather_bands (one grouped point-to-point exchange) or by a GatherRing whose display band is a
    view of the frame (rendered in place)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "3d-renderer_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    import torch.distributed as dist

    import bench
    import oracle_py
    import scene_cases as sc

    dist.init_process_group("gloo", rank=rank, world_size=world)
    scene = getattr(sc, scene_name)()
    W, H = scene.width, scene.height
    bands = bench.band_split(H, world, display_rows)
    spans = [(a * W, (b - a) * W) for a, b in bands]
    col, _, _ = oracle_py.render(scene, band=bands[rank], threads=2)
    mine = torch.from_numpy(np.ascontiguousarray(col).view(np.int32).reshape(-1).copy())
    if ring:
        r = bench.GatherRing(world, spans[rank][1], H * W, lambda n: torch.zeros(n, dtype=torch.int32), rank=rank,
                             spans=spans)
        for k in range(3):  # three frames through the double buffer; the last one is checked
            band = r.acquire()
            if rank == 0:
                assert band.data_ptr() == r.frames[k % 2].data_ptr()  # the display band is the frame's view
            band.copy_(mine if k == 2 else torch.full_like(mine, k))
            r.publish()
        r.drain()
        out = r.frame if rank == 0 else None
    else:
        out = bench.gather_bands(torch.empty(H * W, dtype=torch.int32), mine, world, rank=rank, spans=spans)
    if out is not None:
        np.save(os.path.join(out_dir, "frame.npy"), out.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,display_rows,ring", [(2, 230, False), (3, 200, True), (4, 150, False),
                                                     (4, 90, True)])
def test_uneven_bands_assemble_to_full_frame(world, display_rows, ring, oracle, tmp_path):
    import torch.multiprocessing as mp

    import scene_cases as sc

    mp.start_processes(_uneven_worker, args=(world, _free_port(), "textured_grid", str(tmp_path), display_rows, ring),
                       nprocs=world, join=True, start_method="spawn")
    col, _, _ = oracle.render(sc.textured_grid(), threads=4)
    assert np.array_equal(np.load(tmp_path / "frame.npy"), np.ascontiguousarray(col).view(np.int32).reshape(-1))


class _FakeBand:
    """A stand-in BandRenderer for the autotune logic: step() costs a model time that depends on the
    display-band size and the rank (remote ranks: transfer-bound when their band is large)."""

    def __init__(self, d, rank, H, world, inflight):
        import torch

        self.d, self.rank, self.dev = d, rank, torch.device("cpu")
        rows = d if rank == 0 else (H - d) / (world - 1)
        self.cost = 2e-5 * rows * (1.0 if rank == 0 else 3.0)  # remote: transfer 3x slower per row
        if inflight == 3:  # the model's third frame in flight hides a quarter of the work (well above a loaded
            self.cost *= 0.75  # machine's timing noise: the test runs beside others under pytest -n)
        self.closed = False

    def warm(self):
        pass

    def step(self):
        t = time.perf_counter() + self.cost
        while time.perf_counter() < t:
            pass

    def drain(self):
        pass

    def _sync(self, check=False):
        pass

    def close(self):
        self.closed = True


import time  # noqa: E402


def _autotune_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    import bench

    dist.init_process_group("gloo", rank=rank, world_size=world)
    H = 1000
    made = []

    def make(d, k):
        made.append(_FakeBand(d, rank, H, world, k))
        return made[-1]

    (d, k), log = bench.autotune_split(make, H, world, True, frames=12, rounds=2, warm_seconds=0.01)
    assert all(b.closed for b in made) and len(made) == len(log)
    np.save(os.path.join(out_dir, f"pick{rank}.npy"), np.array([d, k] + [x for x, _, _ in log]))
    dist.barrier()
    dist.destroy_process_group()


def test_autotune_split_picks_the_balanced_display_band(tmp_path):
    """Model: rank 0 costs d rows, each remote rank (H - d) rows at 3x per row (a slow link). The best
    candidate balances them (d = 0.75 H at world 2); every rank picks the same split (max-over-ranks rates)."""
    import torch.multiprocessing as mp

    world = 2
    mp.start_processes(_autotune_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    picks = [np.load(tmp_path / f"pick{r}.npy") for r in range(world)]
    assert np.array_equal(picks[0], picks[1])
    d, k, cands = int(picks[0][0]), int(picks[0][1]), [int(x) for x in picks[0][2:]]
    assert cands == [500, 125, 250, 375, 625, 750] * 2
    assert (d, k) == (750, 3), (d, k, cands)  # 1.5 x the equal band: the balance point


def _codec_worker(rank, world, port, scene_name, out_dir, display_rows, ring, alpha, mode="bgr24", slot=None):
    """A compact band transfer (bench.BandCodec: "bgr24" or "dbp") over gloo: bands packed by the senders, received
    as bytes and unpacked into the display rank's frame, one-shot (gather_bands) or through the double buffer. dbp:
    the slot size is agreed over the ranks (agree_dbp_slot, a max) unless `slot` forces one."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "3d-renderer_amd", "python"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    import torch.distributed as dist

    import bench
    import oracle_py
    import scene_cases as sc

    dist.init_process_group("gloo", rank=rank, world_size=world)
    scene = getattr(sc, scene_name)()
    W, H = scene.width, scene.height
    bands = bench.band_split(H, world, display_rows)
    spans = [(a * W, (b - a) * W) for a, b in bands]
    col, _, _ = oracle_py.render(scene, band=bands[rank], threads=2)
    mine = torch.from_numpy(np.ascontiguousarray(col).view(np.int32).reshape(-1).copy())
    codec = bench.BandCodec(alpha, torch.device("cpu"), mode)
    if mode == "dbp":
        if slot is None:
            bench.agree_dbp_slot(codec, mine, True)
        else:
            codec.slot = slot
    u8 = lambda n: torch.zeros(n, dtype=torch.uint8)  # noqa: E731
    if ring:
        r = bench.GatherRing(world, spans[rank][1], H * W, lambda n: torch.zeros(n, dtype=torch.int32), rank=rank,
                             spans=spans, codec=codec, make_bytes=u8)
        if rank == 0:
            assert r.inbound_bytes == sum(codec.bytes_for(n) for _, n in spans[1:])
        for k in range(3):
            band = r.acquire()
            band.copy_(mine if k == 2 else torch.full_like(mine, ((alpha << 24) | k) - (1 << 32)))
            r.publish()
        r.drain()
        out = r.frame if rank == 0 else None
    else:
        stage = ({q: u8(codec.bytes_for(spans[q][1])) for q in range(1, world)} if rank == 0
                 else u8(codec.bytes_for(spans[rank][1])))
        out = bench.gather_bands(torch.empty(H * W, dtype=torch.int32), mine, world, rank=rank, spans=spans,
                                 codec=codec, stage=stage)
    try:
        codec.check()
        ok = True
    except RuntimeError:
        ok = False
    np.save(os.path.join(out_dir, f"alpha_ok_{rank}.npy"), np.array(ok))
    np.save(os.path.join(out_dir, f"slot_{rank}.npy"), np.array(codec.slot))
    if out is not None:
        np.save(os.path.join(out_dir, "frame.npy"), out.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,display_rows,ring,mode", [(2, None, False, "bgr24"), (3, 200, True, "bgr24"),
                                                          (4, None, True, "bgr24"), (4, 90, False, "bgr24"),
                                                          (2, None, False, "dbp"), (3, 200, True, "dbp"),
                                                          (4, 90, False, "dbp")])
def test_packed_bands_assemble_bit_exact(world, display_rows, ring, mode, oracle, tmp_path):
    """bands sent as 3 bytes per pixel (bgr24) or in the delta bit-plane format (dbp)
    assemble to the same frame as 4-byte bands (the oracle's full frame), when every alpha byte is the promised 255
    (grid_c3: opaque material, tint, white texture and clear colour). dbp: every rank agreed the same slot size."""
    import torch.multiprocessing as mp

    import scene_cases as sc

    mp.start_processes(_codec_worker, args=(world, _free_port(), "grid_c3", str(tmp_path), display_rows, ring, 255,
                                            mode), nprocs=world, join=True, start_method="spawn")
    col, _, _ = oracle.render(sc.grid_c3(), threads=4)
    assert np.array_equal(np.load(tmp_path / "frame.npy"), np.ascontiguousarray(col).view(np.int32).reshape(-1))
    assert all(bool(np.load(tmp_path / f"alpha_ok_{r}.npy")) for r in range(world))
    slots = {int(np.load(tmp_path / f"slot_{r}.npy")) for r in range(world)}
    assert len(slots) == 1
    if mode == "dbp":
        assert slots.pop() < 3 * bench_mod().DBP_SLOT_PIXELS  # smaller than the 3-byte format


def bench_mod():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_dbp_slot_overflow_is_flagged(oracle, tmp_path):
    """A dbp slot too small for a band's content sets the sender's overflow flag (check() raises): a lossy
    transfer cannot pass silently."""
    import torch.multiprocessing as mp

    mp.start_processes(_codec_worker, args=(2, _free_port(), "grid_c3", str(tmp_path), None, False, 255, "dbp",
                                            bench_mod().DBP_HEADER + 16), nprocs=2, join=True, start_method="spawn")
    assert not bool(np.load(tmp_path / "alpha_ok_1.npy"))


def test_packing_a_non_uniform_alpha_is_flagged(oracle, tmp_path):
    """The sender's check: a band whose alpha bytes are not all the promised value (the textured grid's texture
    has alpha) sets the codec's flag, so a lossy 3-byte transfer cannot pass silently."""
    import torch.multiprocessing as mp

    mp.start_processes(_codec_worker, args=(2, _free_port(), "textured_grid", str(tmp_path), None, False, 255),
                       nprocs=2, join=True, start_method="spawn")
    assert not bool(np.load(tmp_path / "alpha_ok_1.npy"))  # rank 1 packed (and flagged) its band


def test_frame_alpha_proof(hiplib):
    """tri_frame_alpha (host-side proof, no GPU needed... but a context needs a device): checked on the GPU in
    test_multidevice_gpu; here the codec's CPU byte shuffle round-trips with the alpha restored."""
    import torch

    import bench

    rng = np.random.default_rng(3)
    px = rng.integers(0, 2 ** 24, 1003, dtype=np.int64)
    band = torch.from_numpy((px | (255 << 24)).astype(np.uint32).view(np.int32))
    codec = bench.BandCodec(255, torch.device("cpu"))
    st = torch.zeros(3 * 1003, dtype=torch.uint8)
    codec.pack(band, st)
    back = torch.zeros_like(band)
    codec.unpack(st, back)
    assert torch.equal(back, band)
    codec.check()
    dbp = bench.BandCodec(255, torch.device("cpu"), "dbp")  # random pixels: the maximum slot, still lossless
    st = torch.zeros(dbp.bytes_for(1003), dtype=torch.uint8)
    dbp.pack(band, st)
    back = torch.zeros_like(band)
    dbp.unpack(st, back)
    assert torch.equal(back, band)
    dbp.check()


def _guard_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist

    import bench

    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cpu")

    def fails_on_rank1():
        if rank == 1:
            raise RuntimeError("tri_xfer_wait: the exchange did not complete before the deadline")
        return {"bad": 0.0, "detail": "ok"}

    res = [bench.guarded_call("check", fails_on_rank1, dev, True, rank, bad=lambda o: o["bad"])]
    res.append(bench.guarded_call("check", lambda: {"bad": float(rank == 0) * 7, "detail": "7 pixels differ"}, dev,
                                  True, rank, bad=lambda o: o["bad"]))
    res.append(bench.guarded_call("check", lambda: (rank, 1), dev, True, rank))
    after = bench.max_over_ranks(float(rank + 10), dev, True)  # the collective sequence is still aligned
    np.save(os.path.join(out_dir, f"guard{rank}.npy"),
            np.array([r[0] for r in res] + [after], dtype=np.float64))
    with open(os.path.join(out_dir, f"guard{rank}.txt"), "w") as f:
        f.write("\n".join(str(r[1]) for r in res))
    dist.destroy_process_group()


def test_guarded_call_agrees_on_a_failure_over_ranks(tmp_path):
    """bench.guarded_call (the fallback guard of the native exchange, VERDICT r5 #1b): an exception on one rank or a
    parity miss on the display rank makes every rank return not-ok from the same single collective, and the ranks'
    collective sequences stay aligned afterwards."""
    import torch.multiprocessing as mp

    world = 2
    mp.start_processes(_guard_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    for r in range(world):
        got = np.load(tmp_path / f"guard{r}.npy")
        assert list(got) == [0.0, 0.0, 1.0, 11.0], (r, got)
    t0 = (tmp_path / "guard0.txt").read_text().splitlines()
    t1 = (tmp_path / "guard1.txt").read_text().splitlines()
    assert "failed on another rank" in t0[0] and "deadline" in t1[0]
    assert "7 pixels differ" in t0[1]
