"""The nearest training graph of N generated graphs: Python sets on the host against ark_graph_nearest on the device
(csrc/graphkey.hip, ark_amd.graphs.nearest):
    python tools/nearest_bench.py [--queries 10000] [--runs 3] [--host-queries 16] [--legs NAME ...]

Legs: the syn-paths, wd-movies and wd-articles presets of ark_amd/datasets.py (entities, relations, triples per graph).  The
training split is uniform random graphs of that shape; of the "generated" rows every second one is a training graph with
about a tenth of its triples redrawn (so that near neighbours exist) and the others are fresh random graphs.  All rows are
token rows made in numpy, seeded; ark_amd.graphs.canon turns them into lists on the device.  Every leg is a child process of
its own under `timeout` (this process never opens the GPU); after the first leg that fails or runs out of time nothing more
is started.  Prints ONE JSON line.

Per leg, after one warm-up, `--runs` timed repetitions (host clock around work that ends in a device synchronise), medians:
  device      graphs.nearest(all queries, all references), strips chosen by the library
  pair_stats  graphs.pair_stats on the enumerated pairs of 64 queries x all references: what a caller had before this kernel;
              reported per 10^6 pairs beside the same figure of `device`
  host        for the FIRST --host-queries queries only: two nested loops over Python sets of the packed triples with exact
              comparison of the fractions (tests/graphnear_ref.nearest_ref), timed once; `host_seconds_extrapolated` scales it
              to all queries and is an extrapolation, not a measurement
The leg fails unless host and device agree on idx, inter, dq and dr of the subsample."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (references, time limit of the leg in seconds)
LEGS = {"syn-paths": (100000, 240), "wd-movies": (100000, 300), "wd-articles": (20000, 420)}
EOS, BOS = 2, 1


def make_rows(name, n_refs, n_queries, seed=0):
    """(reference token rows, query token rows) int64 numpy [*, 3 * max_edges + 2]"""
    import numpy as np
    from ark_amd.datasets import PRESETS
    nE, nR, lo, hi = PRESETS[name]
    ent_base, rel_base = 3, 3 + nE
    rng = np.random.default_rng(seed)

    def triples(rows):
        return np.stack([ent_base + rng.integers(0, nE, (rows, hi)), rel_base + rng.integers(0, nR, (rows, hi)),
                         ent_base + rng.integers(0, nE, (rows, hi))], axis=2)

    def rows_of(tr, k):
        rows = np.full((tr.shape[0], 3 * hi + 2), EOS, dtype=np.int64)
        rows[:, 0] = BOS
        live = np.repeat(np.arange(hi)[None, :] < k[:, None], 3, axis=1)
        rows[:, 1:1 + 3 * hi] = np.where(live, tr.reshape(tr.shape[0], 3 * hi), EOS)
        return rows

    rt, rk = triples(n_refs), rng.integers(lo, hi + 1, n_refs)
    qt, qk = triples(n_queries), rng.integers(lo, hi + 1, n_queries)
    src = rng.integers(0, n_refs, n_queries)
    near = np.arange(n_queries) % 2 == 0
    keep = rng.random((n_queries, hi)) >= 0.1                 # a copied row keeps about nine triples in ten
    qt = np.where((near[:, None] & keep)[:, :, None], rt[src], qt)
    qk = np.where(near, rk[src], qk)
    return rows_of(rt, rk), rows_of(qt, qk)


def host_sets(rows):
    from tests.graphnear_ref import row_sets
    return row_sets(rows)


def run_leg(name, n_queries, runs, host_queries):
    import numpy as np
    import torch
    from ark_amd import graphs
    from tests.graphnear_ref import nearest_ref
    n_refs = LEGS[name][0]
    t0 = time.perf_counter()
    ref_rows, query_rows = make_rows(name, n_refs, n_queries)
    print(f"[nearest_bench] {name}: rows made in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)

    def canon(rows):
        parts = [graphs.canon(torch.from_numpy(rows[i:i + 16384]).cuda(), eos=EOS) for i in range(0, rows.shape[0], 16384)]
        return graphs.GraphBatch(*(torch.cat(x) for x in zip(*parts)))

    refs, queries = canon(ref_rows), canon(query_rows)
    sub = min(64, n_queries)
    both = graphs.GraphBatch(*(torch.cat([q[:sub], r]) for q, r in zip(queries, refs)))
    ia = torch.arange(sub, dtype=torch.int32, device="cuda").repeat_interleave(n_refs)
    ib = (sub + torch.arange(n_refs, dtype=torch.int32, device="cuda")).repeat(sub)

    paths = {"device": lambda: graphs.nearest(queries, refs), "pair_stats": lambda: graphs.pair_stats(both, ia, ib)}
    res = {k: fn() for k, fn in paths.items()}                # warm-up of both paths
    torch.cuda.synchronize()
    secs = {k: [] for k in paths}
    for _ in range(runs):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = fn()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
            print(f"[nearest_bench] {name} {k}: {secs[k][-1]:.4f} s", file=sys.stderr, flush=True)
    near = res["device"]
    summary = graphs.nearest_summary(near)

    hq = min(host_queries, n_queries)
    t0 = time.perf_counter()
    rsets = host_sets(ref_rows)
    sets_s = time.perf_counter() - t0
    qsets = host_sets(query_rows[:hq])
    t0 = time.perf_counter()
    want = nearest_ref(qsets, rsets)
    host_s = time.perf_counter() - t0
    got = [x[:hq].cpu().numpy() for x in near]
    same = all(np.array_equal(g, w) for g, w in zip(got, want))
    # the enumerated pairs give the same winner for the queries both saw
    inter, da, db = (x.view(sub, n_refs)[:hq].cpu().numpy() for x in res["pair_stats"])
    idx = got[0]
    same_pairs = all(inter[q, idx[q]] == got[1][q] and da[q, idx[q]] == got[2][q] and db[q, idx[q]] == got[3][q] for q in range(hq))

    dev = statistics.median(secs["device"])
    pst = statistics.median(secs["pair_stats"])
    out = {"preset": name, "queries": n_queries, "references": n_refs, "cap": int(refs.canon.shape[1]),
           "mean_triples": float(refs.n.double().mean()), "pairs": n_queries * n_refs,
           "device": {"seconds": dev, "seconds_runs": [round(x, 5) for x in secs["device"]],
                      "seconds_per_1e6_pairs": dev / (n_queries * n_refs) * 1e6},
           "pair_stats": {"pairs": sub * n_refs, "seconds": pst, "seconds_runs": [round(x, 5) for x in secs["pair_stats"]],
                          "seconds_per_1e6_pairs": pst / (sub * n_refs) * 1e6},
           "host": {"queries": hq, "seconds": host_s, "reference_sets_seconds": sets_s},
           "host_seconds_extrapolated": host_s * n_queries / max(1, hq),
           "speedup_extrapolated": host_s * n_queries / max(1, hq) / dev,
           "mean_jaccard": summary["mean_jaccard"], "hist": summary["hist"], "copied_rate": summary["copied_rate"],
           "host_equals_device": bool(same), "pair_stats_equals_device": bool(same_pairs)}
    print(json.dumps(out), flush=True)
    assert same and same_pairs, (same, same_pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=3, help="timed repetitions per device path (interleaved)")
    ap.add_argument("--host-queries", type=int, default=16, help="queries of the host leg (the first ones)")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)   # (child mode: run this one leg in this process)
    args = ap.parse_args()
    runs = max(1, args.runs)
    if args.leg:
        run_leg(args.leg, args.queries, runs, args.host_queries)
        return 0
    result = {"tool": "nearest_bench", "queries": args.queries, "runs": runs, "legs": {}}
    rc = 0
    for name in args.legs:
        cmd = ["timeout", "-k", "10", str(LEGS[name][1]), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--queries", str(args.queries), "--runs", str(runs), "--host-queries", str(args.host_queries)]
        print("[nearest_bench]", name, file=sys.stderr, flush=True)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if lines:
            result["legs"][name] = json.loads(lines[-1])
        if p.returncode != 0 or not lines:
            result["legs"].setdefault(name, {})["error"] = f"exit status {p.returncode}"
            result["stopped_after"] = name   # a leg that failed or ran out of time: nothing more is started on the GPU
            rc = 1
            break
    print(json.dumps(result), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
