"""tools/loop_mem_ops.py on a small hand-written listing: the loop is found by its backward branch, its scalar loads,
waits and stores are counted, and the load that reaches a compare in front of a branch is reported."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LISTING = """
\t.text
_Z6k_demoPKv:                           ; @_Z6k_demoPKv
; %bb.0:
\ts_load_dwordx2 s[4:5], s[0:1], 0x0
\ts_waitcnt lgkmcnt(0)
.LBB0_1:                                ; =>This Inner Loop Header
\ts_waitcnt vmcnt(0)
\tds_read_b64 v[2:3], v1
\ts_load_dword s6, s[0:1], 0x10
\ts_waitcnt lgkmcnt(0)
\ts_cmp_eq_u32 s6, 0
\ts_cbranch_scc1 .LBB0_3
; %bb.2:
\ts_load_dwordx4 s[8:11], s[0:1], 0x20
\ts_waitcnt lgkmcnt(0)
\tbuffer_load_dwordx3 v[4:6], v2, s[8:11], 0 idxen
\ts_load_dwordx8 s[12:19], s[0:1], 0x40
\ts_waitcnt vmcnt(0) lgkmcnt(0)
.LBB0_3:
\ts_load_dwordx2 s[20:21], s[0:1], 0x60
\ts_waitcnt lgkmcnt(0)
\tglobal_store_dword v7, v4, s[20:21]
\tglobal_store_dword v7, v5, s[4:5]
\ts_add_i32 s7, s7, -1
\ts_cmp_lg_u32 s7, 0
\ts_cbranch_scc1 .LBB0_1
; %bb.4:
\ts_endpgm
.Lfunc_end0:
"""


def test_loop_counts(tmp_path):
    p = tmp_path / "demo.s"
    p.write_text(LISTING)
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "loop_mem_ops.py"), str(p), "k_demo", "--json"])
    d = json.loads(out)
    assert len(d["loops"]) == 1
    l = d["loops"][0]
    assert l["header"] == ".LBB0_1" and l["blocks"] == 2  # labelled blocks: .LBB0_1 (with its fall-through) and .LBB0_3
    assert l["s_loads"] == 4 and l["s_load_dwords"] == 1 + 4 + 8 + 2  # the load in front of the loop is not counted
    assert l["header_wait"] == "s_waitcnt vmcnt(0)"
    assert l["lgkmcnt0_waits"] == 4 and l["scalar_waits"] == 4 and l["vmcnt0_waits"] == 2
    assert l["vector_loads"] == 1 and l["vector_stores"] == 2
    assert l["s_loads_feeding_branch"] == ["s_load_dword s6, s[0:1], 0x10"]  # the loop counter's compare is not one
    assert l["lgkm_waits_before_first_gather"] == 2 and l["scalar_waits_before_first_gather"] == 2
    assert l["store_tail_sloads"] == 1 and l["post_gather_sloads"] == 2
