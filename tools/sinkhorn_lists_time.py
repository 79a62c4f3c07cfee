"""Times of the Sinkhorn potentials on the candidate lists (kz_softmin_lists.hip) beside the whole-index fit, per shape and K:
(a) the forward search kz_knn for K neighbours, (b) kz_lists_transpose, (c) one column step and (d) one row step with an offset
vector (bytes / time: 12 nnz and 16 n_q K), (e) a ten-iteration kz_sinkhorn_lists call (its own transposition included), (f) the
whole `Sinkhorn(n_iter=10, support="candidates").fit` (uploads, search and (e)); at the first two shapes (g) the whole-index
`Sinkhorn(n_iter=10).fit` on the same embeddings, at 15 000 also (h) the same on the precomputed float32 distance matrix already in
HBM.  float32 euclidean, standard-normal data, temperature 0.02 x the typical distance sqrt(2 d) -- tools/sinkhorn_time.py's setting.
A pair of HIP events around each call (every call ends with a synchronise of the context's stream), one warm-up, the median of
`--reps` (>= 5).  Last: hits@1 of support="candidates" against support="index" on a 15 000 x 15 000 alignment case.

    python tools/sinkhorn_lists_time.py [--out-dir profiles] [--cases small|large|bench|all] [--reps N]

Writes into --out-dir `sinkhorn_lists.jsonl` (one line per shape and K, one for the alignment case; appended) and `sinkhorn_lists.md`:
the tables and the one expectation -- ten list iterations at 15 000 against ten whole-index iterations on the precomputed matrix.
Whatever an existing `sinkhorn_lists.md` holds from its line "## What this says" on is written by hand and kept.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import Kiez, Sinkhorn  # noqa: E402
from kiez_amd import _native as N  # noqa: E402
from tests import sinkhorn_restate as SR  # noqa: E402
from tools.whole_index_time import Events, median_ms  # noqa: E402

# (n_source, n_target, d, the K to run, whole-index fit too, precomputed fit too)
CASES = {"small": [(15_000, 15_000, 300, (10, 50), True, True)], "large": [(100_000, 100_000, 128, (10, 50), True, False)],
         "bench": [(250_000, 1_000_000, 200, (10,), False, False)]}
CASES["all"] = CASES["small"] + CASES["large"] + CASES["bench"]
# profiles/sinkhorn.md: 57 G pairs/s for a whole-index soft-min at 100 000 x 100 000 -- what the projection at the third shape uses
WHOLE_INDEX_PAIRS_PER_S = 57e9


def _fit(s, t, metric, K=10, **hubness_kwargs):
    def run():
        kz = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": metric}, hubness=Sinkhorn,
                  hubness_kwargs=dict(hubness_kwargs))
        kz.fit(s, t)
        kz.hubness.ctx.sync()
        return kz
    return run


def time_case(ctx, ev, rng, reps, n_s, n_t, d, Ks, whole, precomputed):
    s, t = rng.standard_normal((n_s, d)).astype(np.float32), rng.standard_normal((n_t, d)).astype(np.float32)
    sm, tm = N.DeviceMatrix(ctx, s, "euclidean"), N.DeviceMatrix(ctx, t, "euclidean")
    eps = 0.02 * float(np.sqrt(2.0 * d))
    shared = {}
    if whole:
        shared["whole_index_fit_10_iterations_ms"] = round(median_ms(ev, _fit(s, t, "euclidean", temperature=eps, n_iter=10), reps), 2)
    else:
        shared["whole_index_fit_10_iterations_projected_ms"] = round(20 * n_s * n_t / WHOLE_INDEX_PAIRS_PER_S * 1e3, 0)
    if precomputed:
        # the float32 distance matrix, built on the host once and left in HBM: the fit reads it in place
        sq = (s.astype(np.float64) ** 2).sum(axis=1)[:, None] + (t.astype(np.float64) ** 2).sum(axis=1)[None, :]
        D = ctx.to_device(np.sqrt(np.maximum(sq - 2.0 * (s.astype(np.float64) @ t.astype(np.float64).T), 0.0)).astype(np.float32))
        del sq
        shared["precomputed_fit_10_iterations_ms"] = round(median_ms(ev, _fit(D, None, "precomputed", temperature=eps, n_iter=10), reps), 2)
        del D
    lines = []
    for K in Ks:
        dist, ind, _ = N.knn(ctx, sm, tm, K)
        view = N.lists_transpose(ctx, dist, ind, n_t)
        f, g, _, _ = N.sinkhorn_lists(ctx, dist, ind, n_t, eps, 2)
        counts = np.diff(view.colptr.numpy())
        line = {"metric": "euclidean", "dtype": "float32", "n_source": n_s, "n_target": n_t, "d": d, "K": K, "eps": round(eps, 4), "reps": reps,
                "nnz": view.nnz, "longest_column": int(counts.max()), "median_column": float(np.median(counts)),
                "empty_columns": int((counts == 0).sum()),
                "long_columns": int((counts > N.SOFTMIN_LIST_CHUNK).sum()),
                "forward_search_ms": round(median_ms(ev, lambda: N.knn(ctx, sm, tm, K), reps), 3),
                "transpose_ms": round(median_ms(ev, lambda: N.lists_transpose(ctx, dist, ind, n_t), reps), 3),
                "column_step_ms": round(median_ms(ev, lambda: N.softmin_list_cols(ctx, view, eps, off=f), reps), 3),
                "row_step_ms": round(median_ms(ev, lambda: N.softmin_list_rows(ctx, dist, ind, n_t, eps, off=g), reps), 3),
                "sinkhorn_lists_10_iterations_ms": round(median_ms(ev, lambda: N.sinkhorn_lists(ctx, dist, ind, n_t, eps, 10), reps), 3),
                "candidates_fit_10_iterations_ms": round(median_ms(ev, _fit(s, t, "euclidean", K=K, temperature=eps, n_iter=10,
                                                                            support="candidates"), reps), 2)}
        line["column_step_GB_per_s"] = round(12 * view.nnz / line["column_step_ms"] / 1e6, 1)
        line["row_step_GB_per_s"] = round(16 * n_s * K / line["row_step_ms"] / 1e6, 1)
        line.update(shared)
        print(json.dumps(line), flush=True)
        lines.append(line)
        del dist, ind, view, f, g
    return lines


def alignment_line(n=15_000, d=32, noise=1.0, eps=0.02, L=10):
    """hits@1 after `kneighbors(1)` under the raw distance, the whole-index potentials and the list potentials."""
    s, t, gold = SR.alignment_case(n, n, noise, d=d)

    def hits(K, hubness, **kw):
        kz = Kiez(n_candidates=K, algorithm="SklearnNN", algorithm_kwargs={"metric": "cosine"}, hubness=hubness, hubness_kwargs=kw).fit(s, t)
        return round(float((kz.kneighbors(1)[1][:, 0] == gold).mean()), 4), kz
    line = {"alignment_case": [n, n, d, noise], "metric": "cosine", "eps": eps, "n_iter": L, "hits@1_raw_distance": hits(10, None)[0]}
    for K in (10, 50):
        line[f"hits@1_support_index_K{K}"] = hits(K, Sinkhorn, temperature=eps, n_iter=L)[0]
        line[f"hits@1_support_candidates_K{K}"], kz = hits(K, Sinkhorn, temperature=eps, n_iter=L, support="candidates")
        line[f"unlisted_targets_K{K}"] = int(np.isnan(kz.hubness.target_potential_).sum())
    print(json.dumps(line), flush=True)
    return line


def markdown(lines, align):
    ms = lambda x: "—" if x is None else (f"{x:.3f} ms" if x < 10 else f"{x:,.1f} ms".replace(",", " "))   # noqa: E731
    out = ["| shape (n_source × n_target × d) | K | forward search | transposition | column step | row step | `kz_sinkhorn_lists`, 10 it. | "
           "`fit`, support=\"candidates\" | whole-index `fit` | whole-index `fit`, precomputed |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in lines:
        whole = ms(r.get("whole_index_fit_10_iterations_ms")) if "whole_index_fit_10_iterations_ms" in r else \
            f"(projected: {r['whole_index_fit_10_iterations_projected_ms'] / 1e3:.0f} s)"
        out.append(f"| {r['n_source']:,} × {r['n_target']:,} × {r['d']} | {r['K']} | {ms(r['forward_search_ms'])} | {ms(r['transpose_ms'])} | "
                   f"{ms(r['column_step_ms'])} ({r['column_step_GB_per_s']} GB/s) | {ms(r['row_step_ms'])} ({r['row_step_GB_per_s']} GB/s) | "
                   f"{ms(r['sinkhorn_lists_10_iterations_ms'])} | {ms(r['candidates_fit_10_iterations_ms'])} | {whole} | "
                   f"{ms(r.get('precomputed_fit_10_iterations_ms'))} |".replace(",", " "))
    out += ["", "| shape | K | pairs (nnz) | median column | longest column | columns of more than one chunk | empty columns |", "|---|---|---|---|---|---|---|"]
    for r in lines:
        out.append(f"| {r['n_source']:,} × {r['n_target']:,} | {r['K']} | {r['nnz']:,} | {r['median_column']:g} | {r['longest_column']:,} | "
                   f"{r['long_columns']:,} | {r['empty_columns']:,} |".replace(",", " "))
    if align:
        out += ["", "| hits@1, alignment case " + " × ".join(str(x) for x in align["alignment_case"]) + " (cosine, eps "
                f"{align['eps']}, {align['n_iter']} iterations) | raw distance | support=\"index\" | support=\"candidates\" | targets nobody lists |",
                "|---|---|---|---|---|"]
        for K in (10, 50):
            out.append(f"| n_candidates = {K} | {align['hits@1_raw_distance']} | {align[f'hits@1_support_index_K{K}']} | "
                       f"{align[f'hits@1_support_candidates_K{K}']} | {align[f'unlisted_targets_K{K}']} |")
    return "\n".join(out) + "\n"


HAND = "## What this says"
HEAD = """# Sinkhorn on the candidate lists beside the whole-index fit (one MI355X, one box, one process)

`tools/sinkhorn_lists_time.py`: float32 euclidean, standard-normal data, temperature 0.02 × the typical distance √(2d).  A pair of
HIP events around each call (every call ends with a synchronise of the context's stream), one warm-up, the median of 5.  The step
calls run with an offset vector; bytes ÷ time counts 12 bytes per pair for the column step (value and source row) and 16 per entry
for the row step (value and target id); the gathers of the offsets are extra.  `kz_sinkhorn_lists` includes its own transposition;
`fit` includes both uploads, the forward search and that call.  The whole-index fits are `Sinkhorn(n_iter=10).fit` of the same
process on the same data.

## Times (`sinkhorn_lists.jsonl`; `python tools/sinkhorn_lists_time.py --out-dir profiles`)

"""


def expectation(lines):
    """The one expectation: at 15 000 x 15 000 ten list iterations take less than ten whole-index iterations on the precomputed matrix."""
    rows = [r for r in lines if "precomputed_fit_10_iterations_ms" in r]
    if not rows:
        return ""
    out = ["", "Expectation: ten list iterations take less than ten whole-index iterations on the precomputed matrix, same run."]
    for r in rows:
        a, b = r["sinkhorn_lists_10_iterations_ms"], r["precomputed_fit_10_iterations_ms"]
        out.append(f"K = {r['K']}: {a:.3f} ms against {b:.2f} ms -- {'met' if a < b else 'NOT met'} ({b / a:.1f} x).")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-alignment", action="store_true", help="skip the hits@1 comparison")
    args = ap.parse_args()
    reps = max(args.reps, 5)
    ctx = N.Context.get()
    ev = Events()
    rng = np.random.default_rng(0)
    lines = []
    for case in CASES[args.cases]:
        lines += time_case(ctx, ev, rng, reps, *case)
        ctx.trim()
    align = None if args.no_alignment else alignment_line()
    if args.out_dir:
        out = Path(args.out_dir)
        out.mkdir(parents=True, exist_ok=True)
        with open(out / "sinkhorn_lists.jsonl", "a") as f:
            for line in lines + ([align] if align else []):
                f.write(json.dumps(line) + "\n")
        md = out / "sinkhorn_lists.md"
        old = md.read_text() if md.exists() else ""
        tail = old[old.index(HAND):] if HAND in old else ""
        md.write_text(HEAD + markdown(lines, align) + expectation(lines) + "\n" + tail)


if __name__ == "__main__":
    main()
