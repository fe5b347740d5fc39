"""A latent-space walk decoded one latent at a time against one per-latent batched call (Engine.beam_decode_rows, csrc/beam.hip):
    python tools/beam_bench.py [--precision f32] [--latents 600] [--beam 3] [--runs 3] [--legs NAME ...]

Legs: SAIL and t-SAIL at the syn-paths and wd-movies shapes of bench.py's build_cfg, seeded initial weights, N = 600 latents
z ~ N(0, I) -- the 600 points of one flip-rate analysis of kgvae.experiments.interpolation.  Every leg is a child process of
its own under `timeout` (this process never opens the GPU); after the first leg that fails or runs out of time nothing more
is started.  Prints ONE JSON line.

Per leg, with ONE model: after a warm-up of both paths (8 single latents, one batched call), `--runs` timed repetitions,
INTERLEAVED (one at a time, batched, one at a time, ...), each timed by the host clock around work that ends in a device
synchronise:
  one_at_a_time  N calls of decode_latent(z[i:i+1], beam) -- the reference's way, the batch-shared beam on a batch of one;
                 this code path is the parent commit's, untouched
  per_latent     ONE call of decode_latent(z, beam, per_latent=True)
Reported: the median seconds of each, their ratio, library launches and host reads of device tensors of one repetition, and
whether the N decoded graphs were identical."""
# (host reads of the one-at-a-time path are counted on 8 latents and scaled: a counted repetition of all N would double the leg)
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

# name: (model type, workload of bench.py, time limit of the leg in seconds)
LEGS = {
    "SAIL@syn-paths": ("SAIL", "syn-paths", 240),
    "t-SAIL@syn-paths": ("t-SAIL", "syn-paths", 300),
    "SAIL@wd-movies": ("SAIL", "wd-movies", 420),
    "t-SAIL@wd-movies": ("t-SAIL", "wd-movies", 600),
}


def run_leg(name, precision, latents, beam, runs):
    import torch
    import bench
    from sample_bench import _SyncCounter
    from ark_amd import engine as E
    from kgvae.model.models import SAIL
    from kgvae.model.utils import seq_to_triples
    mt, wl, _ = LEGS[name]
    cfg = dict(bench.build_cfg(0.0, wl), model_type=mt, precision=precision)
    torch.manual_seed(0)
    model = SAIL(cfg).to("cuda")
    model.eval()
    z = torch.randn(latents, cfg["d_latent"], generator=torch.Generator().manual_seed(1)).cuda()
    args = (cfg["seq_len"], cfg["special_tokens"], seq_to_triples, cfg["ENT_BASE"], cfg["REL_BASE"])

    def one_at_a_time(n=latents):
        return [model.decode_latent(z[i:i + 1], *args, beam=beam)[0] for i in range(n)]

    def per_latent():
        return model.decode_latent(z, *args, beam=beam, per_latent=True)

    paths = {"one_at_a_time": one_at_a_time, "per_latent": per_latent}
    one_at_a_time(8)
    per_latent()
    torch.cuda.synchronize()
    secs = {k: [] for k in paths}
    launches, graphs = {}, {}
    for _ in range(runs):
        for k, fn in paths.items():
            c0 = E._calls[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            graphs[k] = fn()
            torch.cuda.synchronize()
            secs[k].append(time.perf_counter() - t0)
            launches[k] = E._calls[0] - c0
            print(f"[beam_bench] {name} {k}: {secs[k][-1]:.3f} s", file=sys.stderr, flush=True)
    out = {"model": mt, "workload": wl, "latents": latents, "beam": beam, "seq_len": cfg["seq_len"], "vocab": cfg["vocab_size"],
           "precision": precision, "identical_graphs": graphs["one_at_a_time"] == graphs["per_latent"],
           "differing_latents": sum(a != b for a, b in zip(graphs["one_at_a_time"], graphs["per_latent"]))}
    with _SyncCounter() as one:      # (counted on 8 latents: every latent makes the same reads)
        one_at_a_time(8)
    with _SyncCounter() as rows:
        per_latent()
    reads = {"one_at_a_time": one.n * latents // 8, "per_latent": rows.n}
    for k in paths:
        out[k] = {"seconds": statistics.median(secs[k]), "seconds_runs": [round(x, 4) for x in secs[k]],
                  "library_launches": launches[k], "host_reads": reads[k]}
    out["speedup"] = out["one_at_a_time"]["seconds"] / out["per_latent"]["seconds"]
    out["peak_GiB"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="f32")
    ap.add_argument("--latents", type=int, default=600)
    ap.add_argument("--beam", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3, help="timed repetitions per path (interleaved)")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)   # (child mode: run this one leg in this process)
    args = ap.parse_args()
    runs = max(1, args.runs)
    if args.leg:
        run_leg(args.leg, args.precision, args.latents, args.beam, runs)
        return 0
    result = {"tool": "beam_bench", "precision": args.precision, "latents": args.latents, "beam": args.beam, "runs": runs, "legs": {}}
    rc = 0
    for name in args.legs:
        cmd = ["timeout", "-k", "10", str(LEGS[name][2]), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--precision", args.precision, "--latents", str(args.latents), "--beam", str(args.beam), "--runs", str(runs)]
        print("[beam_bench]", name, file=sys.stderr, flush=True)
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            result["legs"][name] = {"error": f"exit status {p.returncode}"}
            result["stopped_after"] = name   # a leg that failed or ran out of time: nothing more is started on the GPU
            rc = 1
            break
        result["legs"][name] = json.loads(lines[-1])
    print(json.dumps(result), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
