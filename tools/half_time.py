"""Time, memory and results of `fit + kneighbors(10)` on float16 / bfloat16 CUDA tensors resident in HBM, against another build of
the library (the parent commit, which widens such tensors to float64 inside `fit`) on the same tensors, and against the float32
tensors of the same values.  Hubness: CSLS and none.  Shapes: 100 k x 100 k x 768 and 250 k x 1 M x 200.

One call alternates the two libraries `--rounds` times (default three).  Every (library, hubness, input type) of a round is a
fresh process (`--worker --only`): no buffer pool, allocator cache or operand image of one configuration is there for the next.
It draws the tensors from a seeded generator (the same values in every process), runs one warm-up and `--reps` timed repeats --
the host clock around fit + kneighbors, which ends synchronised (the result tensors are cloned on torch's stream and that stream
is synchronised) -- and records the device memory in use (hipMemGetInfo through torch.cuda.mem_get_info) before the first fit and
after the last kneighbors, with the fitted object alive: what the process holds at the end of a step, not a sampled peak.  The
driver prints the spread of the repeats of the SAME library before any difference, and checks that the results of the two
libraries are bit-identical (a SHA-256 of the distance and index bytes).

    python tools/half_time.py --other /path/to/parent/checkout [--labels "this commit,parent"] [--shapes small] [--rounds 3] [--reps 3] [--out FILE.md]
    python tools/half_time.py --worker --root . --shape 250000x1000000x200        (one visit; JSON lines)
    python tools/half_time.py --worker --root . --shape ... --only none:float16 --reps 1   (one configuration: for a kernel trace)
"""
import argparse
import hashlib
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

SHAPES = {"full": ["100000x100000x768", "250000x1000000x200"], "small": ["20000x30000x200"]}
HUBNESS = ("none", "CSLS")
ELEMS = ("float16", "bfloat16", "float32", "float64")     # float64: kernel traces only (the widened copy the parent searches)


def worker(args):
    sys.path.insert(0, str(Path(args.root).resolve()))
    import torch     # first: its HIP runtime is the one the process uses
    import warnings
    from kiez_amd import Kiez
    warnings.simplefilter("ignore")
    n_s, n_t, d = (int(x) for x in args.shape.split("x"))
    g = torch.Generator(device="cuda").manual_seed(0)
    s32 = torch.randn(n_s, d, generator=g, device="cuda", dtype=torch.float32)
    t32 = torch.randn(n_t, d, generator=g, device="cuda", dtype=torch.float32)
    only = [tuple(x.split(":")) for x in args.only.split(",")] if args.only else [(h, e) for h in HUBNESS for e in ELEMS[:3]]
    for hub, elem in only:
        dt = getattr(torch, elem)
        # (the values of the half tensors in every input type: float32 / float64 hold them exactly)
        base = torch.bfloat16 if elem == "bfloat16" else torch.float16
        s = (s32.to(base) if elem in ("float32", "float64") else s32).to(dt).contiguous()
        t = (t32.to(base) if elem in ("float32", "float64") else t32).to(dt).contiguous()
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        times, kz, out = [], None, None
        for rep in range(args.reps + 1):          # (the first one is the warm-up)
            del kz, out
            t0 = time.perf_counter()
            kz = Kiez(n_candidates=10, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness=None if hub == "none" else hub)
            out = kz.fit(s, t).kneighbors(10)
            torch.cuda.synchronize()
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
        free1, _ = torch.cuda.mem_get_info()
        dist, ind = out
        h = hashlib.sha256(dist.cpu().numpy().tobytes())
        h.update(ind.cpu().numpy().tobytes())
        stored = kz.algorithm.target_index
        print(json.dumps({"shape": args.shape, "hubness": hub, "input": elem, "ms": [round(x, 2) for x in times],
                          "used_mib": round((free0 - free1) / 2 ** 20, 1), "input_mib": round((s.nbytes + t.nbytes) / 2 ** 20, 1),
                          "stored_as": getattr(stored, "elem", str(stored.dtype)), "sha256": h.hexdigest()[:16],
                          "dist_dtype": str(dist.dtype)}), flush=True)
        del kz, out, dist, ind, s, t
        # (the next configuration starts from the same footing: neither torch's cache nor the library's buffer pool keeps this one's)
        from kiez_amd import _native as N
        N.Context.get().trim()
        torch.cuda.empty_cache()


def visit(root, shape, reps, hub, elem):
    r = subprocess.run([sys.executable, __file__, "--worker", "--root", str(root), "--shape", shape, "--reps", str(reps), "--only", f"{hub}:{elem}"],
                       capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(f"worker failed in {root} ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=".")
    ap.add_argument("--other", default=None, help="checkout of the build to compare against (built), e.g. the parent commit")
    ap.add_argument("--shape", default=None)
    ap.add_argument("--shapes", default="full", choices=sorted(SHAPES))
    ap.add_argument("--only", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--labels", default="this,other", help="names of the two libraries in the table")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    labels = args.labels.split(",")
    libs = [(labels[0], Path(args.root))] + ([(labels[1], Path(args.other))] if args.other else [])
    lines = ["| shape | hubness | input | library | stored as | ms: median (min .. max of all repeats) | used MiB | input MiB | same bits |",
             "|---|---|---|---|---|---|---|---|---|"]
    for shape in SHAPES[args.shapes]:
        rows = {}      # (hubness, input, library) -> [records of every round]
        for _ in range(args.rounds):
            for hub in HUBNESS:
                for elem in ELEMS[:3]:
                    for name, root in libs:         # alternate the libraries
                        for rec in visit(root, shape, args.reps, hub, elem):
                            rows.setdefault((rec["hubness"], rec["input"], name), []).append(rec)
        for hub in HUBNESS:
            for elem in ELEMS[:3]:
                recs = {name: rows.get((hub, elem, name), []) for name, _ in libs}
                shas = {r["sha256"] for rs in recs.values() for r in rs}
                for name, rs in recs.items():
                    if not rs:
                        continue
                    ms = [x for r in rs for x in r["ms"]]
                    lines.append(f"| {shape} | {hub} | {elem} | {name} | {rs[0]['stored_as']} | {statistics.median(ms):.1f} ({min(ms):.1f} .. {max(ms):.1f}) | "
                                 f"{max(r['used_mib'] for r in rs):.0f} | {rs[0]['input_mib']:.0f} | {'yes' if len(shas) == 1 else 'NO'} |")
                if len(shas) != 1:
                    print(f"RESULTS DIFFER: {shape} {hub} {elem}: {shas}", flush=True)
        print("\n".join(lines), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        Path(args.out).write_text(text)
    ok = "NO |" not in text
    print("results of the two libraries bit-identical on every configuration" if ok else "RESULTS DIFFER (see the table)")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
