"""Sampled generation with the torch sampler against the fused one (`ARK.generate(sampler=...)`, csrc/sample.hip):
    python tools/sample_bench.py [--precision mixed] [--batch 50] [--runs 3] [--legs NAME ...]

Legs: ARK.generate(sample=True, top_p=0.9, batch_size=50) -- the verification call of kgvae.experiments.train -- for ARK and
t-ARK at the syn-paths, wd-movies and wd-articles shapes of bench.py's build_cfg.  Every leg is a child process of its own
under `timeout` (this process never opens the GPU); after the first leg that fails or runs out of time nothing more is
started.  Prints ONE JSON line.

Per leg, with ONE model: after a warm-up generation of 24 positions per sampler, `--runs` whole generations per sampler,
INTERLEAVED (torch, fused, torch, fused, ...), each timed by the host clock around a generation that ends in a device
synchronise; reported per sampler: the median ms per generated token, library launches per token (the engine's C-ABI call
counter: torch's own kernels -- softmax, sort, cumsum, multinomial, cat -- are not in it) and the host synchronisations of
one generation (counted: every bool() / .item() / .cpu() / .tolist() of a device tensor inside generate).  Then the sampler
alone on the leg's own first-step logits [batch, V]: ark_sample_rows against the torch filter chain + multinomial + gather,
device-event time per call over 50 calls each, interleaved three times."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (model type, workload of bench.py, time limit of the leg in seconds)
LEGS = {
    "ARK@syn-paths": ("ARK", "syn-paths", 120),
    "t-ARK@syn-paths": ("t-ARK", "syn-paths", 120),
    "ARK@wd-movies": ("ARK", "wd-movies", 180),
    "t-ARK@wd-movies": ("t-ARK", "wd-movies", 180),
    "ARK@wd-articles": ("ARK", "wd-articles", 300),
    "t-ARK@wd-articles": ("t-ARK", "wd-articles", 300),
}
TOP_P = 0.9


class _SyncCounter:
    """counts the host reads of device tensors while active"""
    NAMES = ("__bool__", "item", "cpu", "tolist")

    def __enter__(self):
        import torch
        self.n, self.saved = 0, {k: getattr(torch.Tensor, k) for k in self.NAMES}
        for k, f in self.saved.items():
            def counted(t, *a, _f=f, **kw):
                if t.is_cuda:
                    self.n += 1
                return _f(t, *a, **kw)
            setattr(torch.Tensor, k, counted)
        return self

    def __exit__(self, *exc):
        import torch
        for k, f in self.saved.items():
            setattr(torch.Tensor, k, f)


def run_leg(name, precision, batch, runs):
    import torch
    import bench
    from ark_amd import engine as E
    from kgvae.model.models import ARK
    mt, wl, _ = LEGS[name]
    cfg = dict(bench.build_cfg(0.0, wl), model_type=mt, precision=precision)
    torch.manual_seed(0)
    model = ARK(cfg).to("cuda")
    model.eval()
    eng = model.engine()
    st, seq_len, V = cfg["special_tokens"], cfg["seq_len"], cfg["vocab_size"]
    steps = {"n": 0}
    def counted(*a, _f=eng.decode_step, **k):
        steps["n"] += 1
        return _f(*a, **k)
    eng.decode_step = counted

    def generate(sampler, length):
        return model.generate(length, st, batch_size=batch, sample=True, top_p=TOP_P, sampler=sampler)

    out = {"model": mt, "workload": wl, "batch": batch, "seq_len": seq_len, "vocab": V, "precision": precision, "top_p": TOP_P}
    samplers = ("torch", "fused")
    for s in samplers:
        generate(s, min(seq_len, 25))
    torch.cuda.synchronize()
    ms = {s: [] for s in samplers}
    tokens, launches = {}, {}
    for _ in range(runs):
        for s in samplers:
            steps["n"] = 0
            c0 = E._calls[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate(s, seq_len)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            tokens[s] = steps["n"]
            launches[s] = (E._calls[0] - c0) / steps["n"]
            ms[s].append(dt * 1e3 / steps["n"])
    for s in samplers:
        with _SyncCounter() as sc:
            generate(s, seq_len)
        out[s] = {"ms_per_token": statistics.median(ms[s]), "ms_per_token_runs": [round(x, 5) for x in ms[s]], "tokens": tokens[s],
                  "library_launches_per_token": round(launches[s], 2), "host_syncs_per_generation": sc.n}
    out["speedup"] = out["torch"]["ms_per_token"] / out["fused"]["ms_per_token"]

    # the sampler alone on this leg's first-step logits
    d = eng.decode_begin(batch)
    logits = eng.decode_step(d, torch.full((batch,), st["BOS"], dtype=torch.int64, device="cuda"), 0).clone()
    tok = torch.zeros(batch, dtype=torch.int64, device="cuda")

    def fused_once(i):
        E.sample_rows(logits, tok, V=V, sample=True, top_p=TOP_P, seed=1, draw=i)

    def torch_once(i):
        _, sp, si = ARK._filter(logits, 1.0, TOP_P, 0)
        si.gather(-1, torch.multinomial(sp, 1))

    def per_call_us(fn, n=50):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn(0)
        torch.cuda.synchronize()
        a.record()
        for i in range(n):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / n

    alone = {"fused": [], "torch": []}
    for _ in range(3):
        alone["torch"].append(per_call_us(torch_once))
        alone["fused"].append(per_call_us(fused_once))
    out["sampler_alone_us"] = {k: statistics.median(v) for k, v in alone.items()}
    out["peak_GiB"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="mixed")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3, help="timed generations per sampler (interleaved); at least 3")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)   # (child mode: run this one leg in this process)
    args = ap.parse_args()
    runs = max(3, args.runs)
    if args.leg:
        run_leg(args.leg, args.precision, args.batch, runs)
        return 0
    result = {"tool": "sample_bench", "precision": args.precision, "batch": args.batch, "runs": runs, "legs": {}}
    rc = 0
    for name in args.legs:
        cmd = ["timeout", "-k", "10", str(LEGS[name][2]), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--precision", args.precision, "--batch", str(args.batch), "--runs", str(runs)]
        print("[sample_bench]", name, file=sys.stderr, flush=True)
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
