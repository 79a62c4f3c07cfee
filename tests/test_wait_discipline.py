"""What a wave of the fp16 sweep kernels waits for between the MFMAs of a tile is written by hand (the slice barrier's
`s_waitcnt vmcnt(0) lgkmcnt(0)`, counted lgkmcnt waits behind the fragment prefetch); hipcc's waitcnt pass adds waits of its own
where it believes a load or a FLAT operation pending, and there `vmcnt` means the LDS-DMA ring.  Checked here on the BUILT device
code: no such wait, no FLAT instruction (tools/check_waits.py)."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import check_waits  # noqa: E402


def listing(name, prog, base=0x1000):
    """A kernel in llvm-objdump's form from instructions, `label:` lines and (branch, label) pairs: objdump prints no local
    labels, a branch's target stands in its comment as <kernel+0xoffset>."""
    addr, at = base, {}
    for p in prog:
        if isinstance(p, str) and p.endswith(":"):
            at[p[:-1]] = addr
        else:
            addr += 4
    lines, addr = [f"{base:016x} <{name}>:"], base
    for p in prog:
        if isinstance(p, str) and p.endswith(":"):
            continue
        if isinstance(p, tuple):
            lines.append(f"\t{p[0]} 1    // {addr:012X}: BF850001 <{name}+0x{at[p[1]] - base:x}>")
        else:
            lines.append(f"\t{p}    // {addr:012X}: 00000000")
        addr += 4
    return "\n".join(lines) + "\n"


MFMA = "v_mfma_f32_32x32x16_f16 v[0:15], v[64:67], v[100:103], v[0:15]"
PROLOGUE = ["global_load_dwordx4 v[100:103], v[2:3], off", "s_waitcnt vmcnt(0)", "ds_write_b32 v1, v100", "s_waitcnt lgkmcnt(0)", "s_barrier",
            "ds_read_b128 v[64:67], v1"]
TAIL = ["global_store_dword v[2:3], v4, off", "s_waitcnt vmcnt(0)", "s_endpgm"]


def kernel(slice2, epilogue, name="kern"):
    """prologue; tile loop = slice 1 (with the barrier and a ring copy), slice 2, epilogue; tail"""
    return listing(name, PROLOGUE + [
        "top:",
        "ds_read_b128 v[68:71], v1 offset:4096", "s_waitcnt lgkmcnt(1)", MFMA, MFMA,
        "s_waitcnt vmcnt(0) lgkmcnt(0)", "s_barrier", "s_mov_b32 m0, s8", "s_nop 0", "global_load_lds_dwordx4 v1, s[2:3]",
    ] + slice2 + epilogue + [("s_cbranch_scc1", "top")] + TAIL)


SLICE2 = ["ds_read_b128 v[64:67], v1 offset:8192", "s_add_i32 s4, s4, 1", "s_waitcnt lgkmcnt(1)", MFMA, MFMA]
# the log flush: skipped by a tile without events; the wait for the atomic's result stands in a block of its own
FLUSH = [("s_cbranch_scc0", "done"), ("s_cbranch_execz", "got"), "global_atomic_add_x2 v[6:7], v5, v[8:9], s[4:5] sc0", "got:",
         "s_waitcnt vmcnt(0)", "global_store_dwordx4 v5, v[10:13], s[6:7] nt", "done:"]
# a merge of a build whose lists live in the output arrays: reads a block of keys back
MERGE = [("s_cbranch_scc0", "done"), "global_load_dwordx4 v[20:23], v5, s[4:5]", "s_waitcnt vmcnt(0)",
         "global_store_dword v5, v20, s[4:5]", "done:"]


def findings(text, spilling=()):
    return [(f[0], f[1]) for f in check_waits.check(text, spilling)[2]]


def test_checker_passes_the_hand_written_waits_and_the_named_exceptions():
    n_k, n_m, bad, allowed = check_waits.check(kernel(SLICE2, FLUSH))
    assert (n_k, n_m, bad) == (1, 4, [])
    assert allowed == {"prologue": 1, "tail": 1, "flush": 1, "merge": 0, "spill": 0, "starved": 0}
    n_k, n_m, bad, allowed = check_waits.check(kernel(SLICE2, MERGE))
    assert bad == [] and allowed["merge"] == 1 and allowed["flush"] == 0


def test_checker_sees_a_vmcnt_wait_between_the_mfmas():
    # a prologue load the pass still believes in flight: awaited at its first use, in every tile -- a wait for the DMA ring
    chain = ["ds_read_b128 v[64:67], v1 offset:8192", "s_waitcnt vmcnt(3) lgkmcnt(1)", MFMA, "s_waitcnt vmcnt(2)", MFMA]
    assert findings(kernel(chain, FLUSH)) == [("kern", "vmcnt")] * 2
    # ... and in front of a tile's first MFMA
    top = kernel(SLICE2, FLUSH).replace("ds_read_b128 v[68:71], v1 offset:4096", "s_waitcnt vmcnt(0)\t\t\t\t")
    assert findings(top) == [("kern", "vmcnt")]
    # a block of the loop that nothing excuses: no flush or merge between it and the last MFMAs
    join = [("s_cbranch_scc0", "done"), "s_add_i32 s4, s4, 1", "done:", "s_waitcnt vmcnt(0)"]
    assert findings(kernel(SLICE2, join)) == [("kern", "vmcnt")]
    # the same wait glued to a barrier is the hand-written one
    assert findings(kernel(SLICE2, join + ["s_barrier"])) == []


def test_checker_sees_a_zero_wait_behind_the_fragment_prefetch():
    zero = ["ds_read_b128 v[64:67], v1 offset:8192", "s_add_i32 s4, s4, 1", "s_waitcnt lgkmcnt(0)", MFMA, MFMA]
    assert findings(kernel(zero, FLUSH)) == [("kern", "lgkm0")]
    # behind an LDS read of the epilogue (no MFMA in the block) it is no prefetch
    epi = [("s_cbranch_scc0", "done"), "ds_read_b128 v[20:23], v5", "s_waitcnt lgkmcnt(0)", "done:"]
    assert findings(kernel(SLICE2, epi)) == []


def test_checker_sees_a_flat_instruction():
    flat = [i.replace("global_store_dwordx4 v5, v[10:13], s[6:7] nt", "flat_store_dwordx4 v[6:7], v[10:13] nt") if isinstance(i, str) else i
            for i in FLUSH]
    assert findings(kernel(SLICE2, flat)) == [("kern", "flat")]


def test_starved_builds_are_excused_by_name_and_only_when_they_spill():
    zero = ["ds_read_b128 v[64:67], v1 offset:8192", "s_waitcnt lgkmcnt(0)", MFMA, MFMA]
    long_list = "_Z20kz_knn_cand_h_kernelILi128ELi7ELi3ELb0EEv13KnnCandParams"
    short_list = "_Z20kz_knn_cand_h_kernelILi16ELi13ELi3ELb1EEv13KnnCandParams"
    for name, spills, want in ((long_list, True, []), (long_list, False, ["lgkm0"]), (short_list, True, ["lgkm0"])):
        text = kernel(zero, FLUSH, name=name)
        assert [f[1] for f in findings(text, {name} if spills else ())] == want
    # a FLAT instruction is excused nowhere
    flat = kernel(zero, ["flat_load_dword v9, v[6:7]"], name=long_list)
    assert [f[1] for f in findings(flat, {long_list})] == ["flat"]


def test_no_compiler_wait_in_the_tile_loops_of_the_built_kernels():
    objs = sorted((ROOT / "kiez_amd" / "csrc").glob("kz_knn_h*.o"))
    if not objs:
        pytest.skip("objects not built (run __graft_entry__.build())")
    mfmas = 0
    for o in objs:
        n_k, n_m, bad, allowed = check_waits.check_object(o)
        assert not bad, (o.name, bad[:5])
        mfmas += n_m
    assert mfmas > 10000   # every build of every fp16 sweep kernel: the check looked at something
