"""Time of the one-to-one matching (kz_match_lists) beside the list call that feeds it, as `Kiez.match_device` runs them: CSLS,
float32 euclidean, lists of `kneighbors_device(k)` and of `kneighbors_whole_index_device(k)`.  Host wall time around each of the
two calls (both end with a synchronise of the context's stream), one warm-up, the best of three.  The data is an alignment task:
every source row is a noisy copy of a target row of its own, on an 8-dimensional subspace so that neighbouring targets get
confused.  One JSON line per (shape, k, whole_index): rounds, matched rows, hits@1 of the lists and the precision of the matching
against the known alignment, the two times and their ratio.

    python tools/match_time.py [--out FILE] [--cases small|medium|large|all]
"""
import argparse
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import Kiez  # noqa: E402
from kiez_amd import _native as N  # noqa: E402

# (n_source, n_target, d, [k ...])
CASES = {"small": [(15_000, 15_000, 300, [10, 100])], "medium": [(100_000, 100_000, 128, [10])],
         "large": [(250_000, 1_000_000, 200, [10])]}
CASES["all"] = CASES["small"] + CASES["medium"] + CASES["large"]
LATENT, NOISE = 8, 0.25


def best_ms(fn, reps=3):
    """(best wall time of `reps` calls after one warm-up, the last call's result)"""
    out = fn()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    args = ap.parse_args()
    ctx = N.Context.get()
    rng = np.random.default_rng(0)
    for n_s, n_t, d, ks in CASES[args.cases]:
        # (rows on an 8-dimensional subspace, the noise inside it: neighbours are close enough for the noise to confuse them --
        #  isotropic noise in d dimensions leaves every source row nearest to its own target, and the matching takes one round)
        basis = rng.standard_normal((LATENT, d), dtype=np.float32)
        z = rng.standard_normal((n_t, LATENT), dtype=np.float32)
        target = z @ basis
        gold = rng.permutation(n_t)[:n_s]
        source = (z[gold] + NOISE * rng.standard_normal((n_s, LATENT), dtype=np.float32)) @ basis
        for k in ks:
            kz = Kiez(n_candidates=k, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS").fit(source, target)
            for whole in (False, True):
                if whole and k > N.KNN_REDUCED_MAX_K:
                    continue

                def lists():
                    out = kz.kneighbors_whole_index_device(k) if whole else kz.kneighbors_device(k)
                    ctx.sync()
                    return out
                list_ms, (dist, ind) = best_ms(lists)
                match_ms, (match, _, rounds) = best_ms(lambda: N.match_lists(ctx, dist, ind, n_t))
                match_h = match.numpy()
                line = {"metric": "euclidean", "dtype": "float32", "hubness": "CSLS", "n_source": n_s, "n_target": n_t, "d": d, "k": k,
                        "whole_index": whole, "rounds": rounds, "matched": int(np.count_nonzero(match_h >= 0)),
                        "hits_at_1_of_lists": round(float(np.mean(ind.numpy()[:, 0] == gold)), 4),
                        "precision_of_matching": round(float(np.mean(match_h == gold)), 4),
                        "list_call_ms": round(list_ms, 3), "match_lists_ms": round(match_ms, 3),
                        "match_over_list_call": round(match_ms / list_ms, 4)}
                print(json.dumps(line), flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
            del kz


if __name__ == "__main__":
    main()
