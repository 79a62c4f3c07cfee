"""Wait discipline of the fp16 sweep kernels (kz_knn_h16.h, kz_knn_hx16.h, kz_knn_h64.h), checked on the BUILT device code.

What the tile loop of those kernels waits for is written by hand: `s_waitcnt vmcnt(0) lgkmcnt(0)` glued to the slice barrier (the
LDS-DMA ring), counted `lgkmcnt` waits that leave the newest fragment prefetch in flight.  hipcc's waitcnt pass adds waits of its
own wherever IT believes something is pending -- and a wait it adds between a tile's MFMAs is a wait for the DMA ring, because
`vmcnt` counts those copies too ("What the waitcnt pass sees").  Three things made it do so, and each is a
finding here, for every kernel of kz_knn_h*.o:

  vmcnt   an `s_waitcnt` with a vmcnt field between two MFMAs that is not glued to an `s_barrier`
          (cause seen: a prologue load the pass still believes in flight at loop entry);
  lgkm0   `s_waitcnt lgkmcnt(0)` directly behind a fragment prefetch (`ds_read_b128` in a block that issues MFMAs; scalar ALU apart)
          (cause seen: a FLAT operation pending -- the pass then waits for zero at every LDS read);
  flat    any `flat_` instruction (it counts in both counters and may return out of order).

Where a vmcnt wait is allowed, by name -- all of them code a tile passes only when it has something to log or to merge, or once:
  prologue  everything in front of the tile loop (the query fragments are loaded and awaited there);
  tail      everything behind the tile loop (the lists go to the output arrays);
  flush     a block without MFMAs behind a `global_atomic_*` or a non-temporal `global_store_*` since the last MFMA block:
            the dual pass' log flush (kz_flush_col3 / kz_flush_col4) awaits the position its atomic reserved;
  merge     a block without MFMAs behind any other `global_*` / `buffer_*` access since the last MFMA block: the list inserts
            of the builds whose lists live in the output arrays (K' = 64, 128) read a block of keys back;
  spill     a wait in a block that itself reloads a spilled register (`scratch_load_*`): tools/spills.py names those kernels --
            a cost that is known and reported there, not one this check may hide or has to repeat.
A block that issues an MFMA is never excused as flush or merge.
One exception is by kernel, not by place:
  starved   vmcnt and lgkm0 findings in a build of kz_knn_cand_h_kernel / kz_knn_cand_hx_kernel with K' >= 64 that SPILLS registers
            (the ELF notes say so; tools/spills.py lists the same kernels).  Those builds have one fragment set or none to spare:
            they read a fragment and wait for it on the spot, or re-read a kernel argument at the top of a tile, because of the
            registers they lack, not because of anything the pass was not told.  Their remedy is a register budget, and no
            flagship route runs them.  They are printed and counted; `flat` findings are never excused.
python3 tools/check_waits.py [-v] [objects...]"""
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from check_m0 import device_disassembly  # noqa: E402
from spills import kernels as register_notes  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
LABEL = re.compile(r"^[0-9a-f]+ <([^>]+)>:")
ADDR = re.compile(r"\s*([0-9A-Fa-f]+):")
TARGET = re.compile(r"<[^>+]+\+0x([0-9a-fA-F]+)>")
BRANCH = re.compile(r"^(s_cbranch|s_branch|s_endpgm|s_setpc|s_swappc)")
MFMA = re.compile(r"^v_(smfmac|mfma)_")
WAIT = re.compile(r"^s_waitcnt\b")
NOP = re.compile(r"^s_(?!waitcnt|barrier)")   # scalar ALU between a read and its wait does not part them
FRAG = re.compile(r"^ds_read_b128\b")
FLAT = re.compile(r"^flat_")
DMA = re.compile(r"^global_load_lds_")
FLUSH = re.compile(r"^global_atomic_|^global_store_.*\bnt\b")
VMEM = re.compile(r"^(global_|buffer_)")
SPILL = re.compile(r"^scratch_load_")
ALLOWED = ("prologue", "tail", "flush", "merge", "spill", "starved")
LONG_LIST = re.compile(r"kz_knn_cand_hx?_kernelILi(64|128)E")


def kernels(text):
    """-> {kernel: (basic blocks [[instruction, ...], ...] in layout order, index of the tile loop's first block, of its last)}.
    llvm-objdump prints no local labels: a branch's target is in its comment (`// address: encoding <kernel+0xoffset>`), so the
    blocks are cut at every branch and every branch target.  The tile loop = the widest backward branch around the first MFMA."""
    out, cur = {}, None
    for line in text.splitlines():
        m = LABEL.match(line)
        if m:
            cur = out.setdefault(m.group(1), {"base": int(line.split()[0], 16), "ins": []})
            continue
        ins, _, note = line.partition("//")
        ins = ins.strip()
        a = ADDR.match(note)
        if not ins or cur is None or not a:
            continue
        t = TARGET.search(note) if BRANCH.match(ins) else None
        cur["ins"].append((int(a.group(1), 16), ins, cur["base"] + int(t.group(1), 16) if t else None))
    res = {}
    for name, k in out.items():
        ins = k["ins"]
        cuts = {t for _, _, t in ins if t is not None}
        blocks, starts, new = [], [], True
        for addr, i, _ in ins:
            if new or addr in cuts:
                blocks.append([])
                starts.append(addr)
            blocks[-1].append(i)
            new = bool(BRANCH.match(i))
        mf = [addr for addr, i, _ in ins if MFMA.match(i)]
        lo = hi = None
        if mf:
            back = [(t, addr) for addr, _, t in ins if t is not None and t <= mf[0] <= addr]
            if back:
                lo, hi = min(t for t, _ in back), max(a_ for _, a_ in back)
        block_of = lambda x: None if x is None else max(i for i, s_ in enumerate(starts) if s_ <= x)  # noqa: E731
        res[name] = (blocks, block_of(lo), block_of(hi))
    return res


def check_kernel(blocks, loop_first=None, loop_last=None):
    """-> (findings [(kind, instruction context)], allowed {name: count}, MFMAs)"""
    has_mfma = [any(MFMA.match(i) for i in b) for b in blocks]
    n_mfma = sum(sum(1 for i in b if MFMA.match(i)) for b in blocks)
    findings, allowed = [], dict.fromkeys(ALLOWED, 0)
    for b in blocks:
        findings += [("flat", i) for i in b if FLAT.match(i)]
    if not n_mfma:
        return findings, allowed, 0
    # (a kernel without a loop around its MFMAs: from the first block that issues one to the last)
    first = has_mfma.index(True) if loop_first is None else loop_first
    last = len(blocks) - 1 - has_mfma[::-1].index(True) if loop_last is None else loop_last
    region = None   # what the blocks since the last MFMA block have done: None, "merge" or "flush"
    for bi, b in enumerate(blocks):
        if has_mfma[bi]:
            region = None
        for k, ins in enumerate(b):
            if not has_mfma[bi] and not DMA.match(ins):
                if FLUSH.match(ins):
                    region = "flush"
                elif VMEM.match(ins) and region is None:
                    region = "merge"
            if not WAIT.match(ins):
                continue
            glued = k + 1 < len(b) and b[k + 1].startswith("s_barrier")
            prev = next((p for p in reversed(b[:k]) if not NOP.match(p)), "")
            if "lgkmcnt(0)" in ins and not glued and has_mfma[bi] and FRAG.match(prev):
                findings.append(("lgkm0", f"{prev} ; {ins}"))
            if "vmcnt" not in ins or glued:
                continue
            if bi < first:
                allowed["prologue"] += 1
            elif bi > last:
                allowed["tail"] += 1
            elif any(SPILL.match(p) for p in b[:k]):
                allowed["spill"] += 1
            elif not has_mfma[bi] and region:
                allowed[region] += 1
            else:
                findings.append(("vmcnt", f"{ins} (block {bi}{', issues MFMAs' if has_mfma[bi] else ''})"))
    return findings, allowed, n_mfma


def check(text, spilling=()):
    """-> (kernels with MFMAs, MFMAs, findings [(kernel, kind, context)], allowed {name: count}); spilling = names of the kernels
    that spill registers"""
    n_k, n_m, findings, allowed = 0, 0, [], dict.fromkeys(ALLOWED, 0)
    for name, (blocks, lo, hi) in kernels(text).items():
        f, a, m = check_kernel(blocks, lo, hi)
        if name in spilling and LONG_LIST.search(name):
            a["starved"] = sum(1 for x in f if x[0] != "flat")
            f = [x for x in f if x[0] == "flat"]
        n_k += m > 0
        n_m += m
        findings += [(name,) + x for x in f]
        for k, v in a.items():
            allowed[k] += v
    return n_k, n_m, findings, allowed


def check_object(obj):
    return check(device_disassembly(obj), {k[0] for k in register_notes(obj) if k[2] or k[3]})


def main(argv):
    verbose = "-v" in argv
    objs = [Path(a) for a in argv if a != "-v"] or sorted((ROOT / "kiez_amd" / "csrc").glob("kz_knn_h*.o"))
    total, failures = 0, []
    for o in objs:
        n_k, n_m, findings, allowed = check_object(o)
        total += n_m
        failures += [(o.name,) + f for f in findings]
        kinds = {k: sum(1 for f in findings if f[1] == k) for k in ("vmcnt", "lgkm0", "flat")}
        print(f"{o.name}: {n_k} kernels, {n_m} MFMAs; findings {kinds}; allowed vmcnt waits {allowed}")
    for f in failures[: None if verbose else 20]:
        print("  FINDING", f)
    print("MFMAs walked:", total, " findings:", len(failures))
    return 1 if failures or total == 0 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
