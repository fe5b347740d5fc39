"""Counting the distinct graphs among N generated token rows: the host path against graph keys on the device (csrc/graphkey.hip):
    python tools/graphkey_bench.py [--rows 10000] [--runs 3] [--legs NAME ...]

Legs: SAIL at the syn-paths, wd-movies and wd-articles shapes of bench.py's build_cfg, seeded initial weights, precision f32,
N = 10 000 rows sampled from latents z ~ N(0, I) with the fused sampler (SAIL.sample_latent, seeded; generated once per leg,
in batches, and timed on its own).  Every leg is a child process of its own under `timeout` (this process never opens the
GPU); after the first leg that fails or runs out of time nothing more is started.  Prints ONE JSON line.

Per leg, `--runs` timed repetitions of both paths over the SAME device tensor of tokens, INTERLEAVED (host, device, host, ...),
each timed by the host clock around work that ends in a device synchronise, after one warm-up of each:
  host    toks.cpu(), seq_to_triples per row, canonical_graph_string, a Python set -- what SAIL.count_unique_graphs and the
          verification block of kgvae.experiments.train do with decoded rows; this code is the parent commit's, untouched
  device  ark_amd.graphs.canon (one ark_graph_canon launch) and unique_count (two sorts on the [N, 2] keys), one host read
Reported: the median seconds of each, their ratio, the seconds of the key kernel alone, and the two unique counts, which must
be equal (the leg fails otherwise)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (workload of bench.py, latents per generation batch, time limit of the leg in seconds)
LEGS = {
    "syn-paths": ("syn-paths", 10000, 180),
    "wd-movies": ("wd-movies", 5000, 300),
    "wd-articles": ("wd-articles", 1000, 540),
}


def run_leg(name, rows, runs):
    import torch
    import bench
    from ark_amd import graphs
    from kgvae.model.models import SAIL
    from kgvae.model.utils import canonical_graph_string, seq_to_triples
    wl, gen_batch, _ = LEGS[name]
    cfg = dict(bench.build_cfg(0.0, wl), precision="f32")
    st, eb, rb = cfg["special_tokens"], cfg["ENT_BASE"], cfg["REL_BASE"]
    torch.manual_seed(0)
    model = SAIL(cfg).to("cuda")
    model.eval()
    z = torch.randn(rows, cfg["d_latent"], generator=torch.Generator().manual_seed(1)).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    toks = torch.cat([model.sample_latent(z[i:i + gen_batch], cfg["seq_len"], st, sample=True, seed=2 + i)
                      for i in range(0, rows, gen_batch)])
    torch.cuda.synchronize()
    gen_s = time.perf_counter() - t0
    print(f"[graphkey_bench] {name}: {rows} rows of {toks.shape[1]} tokens generated in {gen_s:.2f} s", file=sys.stderr, flush=True)

    def host():
        graphs_ = [seq_to_triples(row, st, eb, rb) for row in toks.cpu()]
        return len({canonical_graph_string(g) for g in graphs_})

    def device():
        return graphs.unique_count(graphs.canon(toks, None, eos=st["EOS"], vocab=cfg["vocab_size"]))

    def kernel():
        graphs.canon(toks, None, eos=st["EOS"], vocab=cfg["vocab_size"])
        return None

    paths = {"host": host, "device": device, "kernel": kernel}
    counts = {k: fn() for k, fn in paths.items()}          # warm-up of every path
    torch.cuda.synchronize()
    secs = {k: [] for k in paths}
    for _ in range(runs):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            counts[k] = fn()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
            print(f"[graphkey_bench] {name} {k}: {secs[k][-1]:.4f} s", file=sys.stderr, flush=True)
    batch = graphs.canon(toks, None, eos=st["EOS"], vocab=cfg["vocab_size"])
    out = {"workload": wl, "rows": rows, "seq_len": cfg["seq_len"], "row_len": int(toks.shape[1]), "vocab": cfg["vocab_size"],
           "generate_seconds": gen_s, "unique_host": counts["host"], "unique_device": counts["device"],
           "mean_triples": float(batch.n.double().mean()), "empty": int((batch.n == 0).sum())}
    for k in paths:
        out[k] = {"seconds": statistics.median(secs[k]), "seconds_runs": [round(x, 5) for x in secs[k]]}
    out["speedup"] = out["host"]["seconds"] / out["device"]["seconds"]
    print(json.dumps(out), flush=True)
    assert counts["host"] == counts["device"], (counts["host"], counts["device"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--runs", type=int, default=3, help="timed repetitions per path (interleaved)")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)   # (child mode: run this one leg in this process)
    args = ap.parse_args()
    runs = max(1, args.runs)
    if args.leg:
        run_leg(args.leg, args.rows, runs)
        return 0
    result = {"tool": "graphkey_bench", "precision": "f32", "rows": args.rows, "runs": runs, "legs": {}}
    rc = 0
    for name in args.legs:
        cmd = ["timeout", "-k", "10", str(LEGS[name][2]), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--rows", str(args.rows), "--runs", str(runs)]
        print("[graphkey_bench]", name, file=sys.stderr, flush=True)
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
