"""Time of the minimum-cost assignment (kz_assign_lists) beside the list call that feeds it, as `Kiez.assign_device` runs them, and
beside the stable matching on the same lists: CSLS, float32 euclidean, lists of `kneighbors_device(k)` and of
`kneighbors_whole_index_device(k)`; the data generator and the shapes of tools/match_time.py.  Host wall time around each call
(all end with a synchronise of the context's stream), one warm-up, the best of three.  `unmatched_cost` and `eps` are the defaults
of `matching.assignment` unless `--u-frac` places `unmatched_cost` inside the range of the listed values.  One JSON line per
(shape, k, whole_index): rounds, matched rows, the total cost (matched values plus unmatched_cost per unmatched row) and the
precision against the known alignment of the assignment and of the stable matching, the time of the list call, of
kz_assign_lists with the default switch to the single-workgroup kernel and with `tail_rows = -1` (grid-wide rounds only), and of
kz_match_lists.

    python tools/assign_time.py [--out FILE] [--cases small|medium|large|all] [--u-frac F] [--no-wide-only] [--max-rounds N] [--k K]
"""
import argparse
import json
import sys

import numpy as np

sys.path.insert(0, ".")
from kiez_amd import Kiez  # noqa: E402
from kiez_amd import _native as N  # noqa: E402
from kiez_amd import matching  # noqa: E402
from tools.match_time import CASES, LATENT, NOISE, best_ms  # noqa: E402


def total_cost(dist, col, u):
    on = col >= 0
    return float(dist[np.nonzero(on)[0], col[on]].astype(np.float64).sum() + u * np.count_nonzero(~on))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cases", default="all", choices=sorted(CASES))
    ap.add_argument("--u-frac", type=float, default=None, help="unmatched_cost = min + F * (max - min) of the listed values")
    ap.add_argument("--no-wide-only", action="store_true", help="skip the tail_rows = -1 run")
    ap.add_argument("--max-rounds", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=None, help="only this k of the chosen cases")
    args = ap.parse_args()
    ctx = N.Context.get()
    rng = np.random.default_rng(0)
    for n_s, n_t, d, ks in CASES[args.cases]:
        basis = rng.standard_normal((LATENT, d), dtype=np.float32)
        z = rng.standard_normal((n_t, LATENT), dtype=np.float32)
        target = z @ basis
        gold = rng.permutation(n_t)[:n_s]
        source = (z[gold] + NOISE * rng.standard_normal((n_s, LATENT), dtype=np.float32)) @ basis
        for k in ks if args.k is None else [k for k in ks if k == args.k]:
            kz = Kiez(n_candidates=k, algorithm="SklearnNN", algorithm_kwargs={"metric": "euclidean"}, hubness="CSLS").fit(source, target)
            for whole in (False, True):
                if whole and k > N.KNN_REDUCED_MAX_K:
                    continue

                def lists():
                    out = kz.kneighbors_whole_index_device(k) if whole else kz.kneighbors_device(k)
                    ctx.sync()
                    return out
                list_ms, (dist, ind) = best_ms(lists)
                lo, hi = N.assign_range(ctx, dist, ind, n_t)
                u, eps = matching._assignment_defaults((lo, hi), n_s, None if args.u_frac is None else lo + args.u_frac * (hi - lo), None)
                assign_ms, (_, col, _, rounds, converged) = best_ms(lambda: N.assign_lists(ctx, dist, ind, n_t, u, eps, args.max_rounds))
                wide_ms = None
                if not args.no_wide_only and converged and rounds <= 1_000_000:   # (three launches a round: one timed run where the rounds are many)
                    wide_ms, (_, col_w, _, rounds_w, _) = best_ms(lambda: N.assign_lists(ctx, dist, ind, n_t, u, eps, args.max_rounds, tail_rows=-1),
                                                                  reps=3 if rounds <= 100_000 else 1)
                    assert rounds_w == rounds and np.array_equal(col_w.numpy(), col.numpy())
                match_ms, (_, col_s, rounds_s) = best_ms(lambda: N.match_lists(ctx, dist, ind, n_t))
                dist_h, ind_h, col_h, col_sh = dist.numpy(), ind.numpy(), col.numpy(), col_s.numpy()
                rows = np.arange(n_s)

                def precision(c):
                    return round(float(np.mean(np.where(c >= 0, ind_h[rows, np.maximum(c, 0)], -1) == gold)), 4)
                line = {"metric": "euclidean", "dtype": "float32", "hubness": "CSLS", "n_source": n_s, "n_target": n_t, "d": d, "k": k,
                        "whole_index": whole, "unmatched_cost": u, "eps": eps, "rounds": rounds, "converged": converged,
                        "matched": int(np.count_nonzero(col_h >= 0)), "cost": round(total_cost(dist_h, col_h, u), 4),
                        "precision": precision(col_h), "stable_rounds": rounds_s, "stable_matched": int(np.count_nonzero(col_sh >= 0)),
                        "stable_cost": round(total_cost(dist_h, col_sh, u), 4), "stable_precision": precision(col_sh),
                        "hits_at_1_of_lists": round(float(np.mean(ind_h[:, 0] == gold)), 4),
                        "list_call_ms": round(list_ms, 3), "assign_lists_ms": round(assign_ms, 3),
                        "assign_lists_wide_only_ms": None if wide_ms is None else round(wide_ms, 3), "match_lists_ms": round(match_ms, 3),
                        "us_per_round": round(assign_ms * 1e3 / max(rounds, 1), 3),
                        "us_per_round_wide_only": None if wide_ms is None else round(wide_ms * 1e3 / max(rounds, 1), 3)}
                print(json.dumps(line), flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
            del kz


if __name__ == "__main__":
    main()
