#!/usr/bin/env python3
"""Scalar-memory traffic of each loop of one kernel in a gfx950 assembly listing (hipcc -S --cuda-device-only).

  python tools/loop_mem_ops.py listing.s KERNEL_SUBSTRING [--json] [--min-vmem N] [--show LABEL]

A loop is the run of basic blocks from a backward branch's target to the branch (inner loops are listed on their
own and counted again inside the loops around them). Per loop: the scalar loads, the s_waitcnt (those that drain
the scalar/LDS counter, lgkmcnt(0), and those that drain the vector-memory counter, vmcnt(0), apart; `scalar_waits`
are the lgkmcnt(0) waits with a scalar load of the loop outstanding, i.e. the serial scalar round trips), the vector
loads and stores, and the scalar loads that feed a branch: a load whose result reaches, through scalar ALU
instructions only, a compare or a mask test in front of an s_cbranch of the same loop. `header_wait` is the first
s_waitcnt of the loop; `lgkm_waits_before_first_gather` counts the lgkmcnt(0) waits between the loop's first LDS read
and its first vector load (`scalar_waits_before_first_gather`: those with a scalar load outstanding);
`store_tail_sloads` the scalar loads that stand in a block with a vector store, in front of its last store
(`post_gather_sloads`: all scalar loads after the loop's last vector load). The blocks are read in layout order, so a
side block the compiler placed inside the loop counts with it. After the loops: the kernel's registers, scratch
bytes (spilled VGPRs) and LDS bytes from its .amdhsa block and the compiler's remarks; `readlanes` / `writelanes`
per loop are the SGPRs spilled to VGPR lanes that the loop reloads and saves.
--show LABEL prints that loop's instructions with the loads, waits and branches marked."""
import json
import re
import sys

SREG = re.compile(r"\b(s\[\d+:\d+\]|s\d+|vcc|scc|exec)\b")


def kernel_lines(path, name):
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*:", l) and name in l.split(":")[0])
    end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines, start, end


def expand(reg):
    m = re.match(r"s\[(\d+):(\d+)\]", reg)
    if m:
        return {f"s{i}" for i in range(int(m.group(1)), int(m.group(2)) + 1)}
    return {reg}


def operands(s):
    body = s.split(";")[0]
    parts = body.split(None, 1)
    if len(parts) < 2:
        return []
    return [o.strip() for o in parts[1].split(",")]


def regs_of(ops):
    out = set()
    for o in ops:
        for r in SREG.findall(o):
            out |= expand(r)
    return out


def parse_blocks(lines, start, end):
    blocks, cur = [], {"label": "entry", "ins": []}
    for l in lines[start + 1:end]:
        s = l.strip()
        m = re.match(r"^(\.LBB\S+):", s)
        if m:
            blocks.append(cur)
            cur = {"label": m.group(1), "ins": []}
            continue
        if not s or s.startswith((";", ".")):
            continue
        cur["ins"].append(s.split(";")[0].strip())
    blocks.append(cur)
    return blocks


def find_loops(blocks):
    index = {b["label"]: i for i, b in enumerate(blocks)}
    loops = {}
    for i, b in enumerate(blocks):
        for ins in b["ins"]:
            if ins.startswith(("s_cbranch", "s_branch")):
                m = re.search(r"(\.LBB\S+)", ins)
                if m and index.get(m.group(1), 1 << 30) <= i:
                    h = index[m.group(1)]
                    loops[h] = max(loops.get(h, h), i)
    return sorted(loops.items())


def is_sload(op):
    return op.startswith(("s_load_", "s_buffer_load_"))


def is_vload(op):
    return op.startswith(("buffer_load", "global_load", "flat_load", "scratch_load"))


def is_vstore(op):
    return op.startswith(("buffer_store", "global_store", "flat_store", "scratch_store"))


def analyse(blocks, h, t):
    ins = [(blocks[i]["label"], s) for i in range(h, t + 1) for s in blocks[i]["ins"]]
    r = {"header": blocks[h]["label"], "blocks": t - h + 1, "instructions": len(ins), "s_loads": 0, "s_load_dwords": 0,
         "s_waitcnt": 0, "lgkmcnt0_waits": 0, "scalar_waits": 0, "vmcnt0_waits": 0, "vector_loads": 0, "vector_stores": 0, "lds_reads": 0,
         "branches": 0, "s_loads_feeding_branch": [], "header_wait": None, "lgkm_waits_before_first_gather": None,
         "scalar_waits_before_first_gather": None,
         "store_tail_sloads": 0, "post_gather_sloads": 0, "scratch_ops": 0, "readlanes": 0, "writelanes": 0}
    taint = {}  # sgpr -> the scalar load it descends from
    flag = {}   # scc / vcc -> load
    seen_lds, seen_gather, waits_before, swaits_before, pending = False, False, 0, 0, 0
    last_vload = max((k for k, (_, s) in enumerate(ins) if is_vload(s.split()[0])), default=-1)
    for i in range(h, t + 1):  # the store tail: scalar loads in front of the last store of a storing block
        ops_i = [s.split()[0] for s in blocks[i]["ins"]]
        stores = [k for k, o in enumerate(ops_i) if is_vstore(o) and not o.startswith("scratch_")]
        if stores:
            r["store_tail_sloads"] += sum(is_sload(o) for o in ops_i[:stores[-1]])
    for k, (_, s) in enumerate(ins):
        op = s.split()[0]
        ops = operands(s)
        if is_sload(op):
            r["s_loads"] += 1
            pending += 1
            m = re.search(r"dwordx(\d+)", op)
            r["s_load_dwords"] += int(m.group(1)) if m else 1
            for d in regs_of(ops[:1]):
                taint[d] = s
            if last_vload >= 0 and k > last_vload:
                r["post_gather_sloads"] += 1
        elif op == "s_waitcnt":
            r["s_waitcnt"] += 1
            if r["header_wait"] is None:
                r["header_wait"] = s
            if "lgkmcnt(0)" in s:
                r["lgkmcnt0_waits"] += 1
                r["scalar_waits"] += pending > 0
                if seen_lds and not seen_gather:
                    waits_before += 1
                    swaits_before += pending > 0
                pending = 0
            if "vmcnt(0)" in s:
                r["vmcnt0_waits"] += 1
        elif is_vload(op):
            r["vector_loads"] += 1
            r["scratch_ops"] += op.startswith("scratch_")
            if not seen_gather and not op.startswith("scratch_"):
                seen_gather = True
                r["lgkm_waits_before_first_gather"] = waits_before
                r["scalar_waits_before_first_gather"] = swaits_before
        elif is_vstore(op):
            r["vector_stores"] += 1
            r["scratch_ops"] += op.startswith("scratch_")
        elif op.startswith("ds_read") or op.startswith("ds_load"):
            r["lds_reads"] += 1
            seen_lds = True
        elif op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
            r["readlanes"] += op.startswith("v_readlane")
            for d in regs_of(ops[:1]):
                taint.pop(d, None)
        elif op.startswith("v_writelane"):
            r["writelanes"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            r["branches"] += 1
            src = None
            if "scc" in op:
                src = flag.get("scc")
            elif "vcc" in op:
                src = flag.get("vcc")
            if src and src not in r["s_loads_feeding_branch"]:
                r["s_loads_feeding_branch"].append(src)
        elif op.startswith("s_"):
            used = regs_of(ops[1:]) if not op.startswith(("s_cmp", "s_bitcmp")) else regs_of(ops)
            src = next((taint[u] for u in sorted(used) if u in taint), None)
            if op.startswith(("s_cmp", "s_bitcmp")):
                flag["scc"] = src
            else:
                dst = regs_of(ops[:1])
                for d in dst:
                    if src:
                        taint[d] = src
                    else:
                        taint.pop(d, None)
                if "vcc" in dst:
                    flag["vcc"] = src
                # logical and arithmetic scalar instructions set SCC from their result
                if re.match(r"s_(and|or|xor|andn2|orn2|nand|nor|xnor|add|sub|lshl|lshr|ashr|min|max|abs|not|bfe)", op):
                    flag["scc"] = src
        elif op.startswith("v_cmp") and ops and "vcc" in regs_of(ops[:1]):
            flag["vcc"] = None
    return r


def kernel_meta(lines, start, end, name):
    meta = {}
    for i, l in enumerate(lines):
        if l.strip().startswith(".amdhsa_kernel") and name in l:
            for m in lines[i:i + 60]:
                mm = re.match(r"\s*\.amdhsa_(group_segment_fixed_size|private_segment_fixed_size|next_free_vgpr|next_free_sgpr)\s+(\S+)", m)
                if mm:
                    meta[mm.group(1)] = int(mm.group(2)) if mm.group(2).isdigit() else mm.group(2)
                if ".end_amdhsa_kernel" in m:
                    break
    for i, l in enumerate(lines):  # the code object's metadata: spill counts
        if re.match(r"\s*\.name:\s", l) and name in l:
            for m in lines[i:i + 14]:
                mm = re.match(r"\s*\.(sgpr_count|sgpr_spill_count|vgpr_count|vgpr_spill_count):\s*(\d+)", m)
                if mm:
                    meta[mm.group(1)] = int(mm.group(2))
    for l in lines[end:end + 60]:
        mm = re.match(r";\s*(SGPRBlocks|VGPRBlocks|NumSgprs|NumVgprs|ScratchSize|Occupancy|sgpr_spill_count|vgpr_spill_count|LDSByteSize|SGPRs|VGPRs|SGPR spill count|VGPR spill count)\s*:?\s*(\d+)", l.strip(), re.I)
        if mm:
            meta[mm.group(1)] = int(mm.group(2))
    return meta


def main():
    path, name = sys.argv[1], sys.argv[2]
    as_json = "--json" in sys.argv
    min_vmem = int(sys.argv[sys.argv.index("--min-vmem") + 1]) if "--min-vmem" in sys.argv else 0
    show = sys.argv[sys.argv.index("--show") + 1] if "--show" in sys.argv else None
    lines, start, end = kernel_lines(path, name)
    blocks = parse_blocks(lines, start, end)
    loops = [analyse(blocks, h, t) for h, t in find_loops(blocks)]
    loops = [l for l in loops if l["vector_loads"] + l["vector_stores"] >= min_vmem]
    meta = kernel_meta(lines, start, end, name)
    if show:
        idx = {b["label"]: i for i, b in enumerate(blocks)}
        h = idx[show]
        t = dict(find_loops(blocks))[h]
        for i in range(h, t + 1):
            print(blocks[i]["label"] + ":")
            for s in blocks[i]["ins"]:
                op = s.split()[0]
                mark = "S" if is_sload(op) else "W" if op == "s_waitcnt" else "B" if op.startswith(("s_cbranch", "s_branch")) else \
                       "L" if is_vload(op) else "T" if is_vstore(op) else "D" if op.startswith("ds_") else " "
                if mark != " ":
                    print(f"  {mark} {s}")
        return
    if as_json:
        print(json.dumps({"kernel": lines[start].split(":")[0], "meta": meta, "loops": loops}, indent=1))
        return
    print(lines[start].split(":")[0])
    for l in loops:
        print(f"{l['header']:<12} blocks {l['blocks']:3d} ins {l['instructions']:5d}  s_load {l['s_loads']:3d} ({l['s_load_dwords']} dw)"
              f"  waitcnt {l['s_waitcnt']:3d} (lgkm0 {l['lgkmcnt0_waits']}, scalar {l['scalar_waits']}, vm0 {l['vmcnt0_waits']})  vload {l['vector_loads']:3d}"
              f" vstore {l['vector_stores']:2d}  loads->branch {len(l['s_loads_feeding_branch'])}"
              f"  lgkm0 before gathers {l['lgkm_waits_before_first_gather']} (scalar {l['scalar_waits_before_first_gather']})  tail s_loads {l['store_tail_sloads']} (after gathers {l['post_gather_sloads']})"
              f"  lanes r{l['readlanes']}/w{l['writelanes']} scratch {l['scratch_ops']}  header wait: {l['header_wait']}")
    print("meta", meta)


if __name__ == "__main__":
    main()
