"""Greedy / beam generation of the Transformer variants with the K/V-cache decoder (`ark_txf_kv_cache`) on and off:
    python tools/decode_bench.py [--precision mixed] [--batch 64] [--legs NAME ...] [--no-kernel-time]

Legs: t-ARK ARK.generate, t-SAIL decode_latent with beam 1 and beam 4, batch 64, at the syn-paths and wd-articles shapes bench.py
uses for the Transformer variants.  Every leg is a child process of its own under `timeout` (this process never opens the
GPU); inside a leg ONE model generates with the switch on and with it off (the prefix re-run: the reference's algorithm, and
what the parent of this change ran).  After the first leg that fails or runs out of time nothing more is started.

Prints ONE JSON line.  Per leg and path: ms per generated token (host clock around whole generations that end in a device
synchronise, after a short warm-up generation of 24 positions that loads every kernel and allocates the workspaces), library
launches per token (the engine's C-ABI call counter; torch's own small kernels -- argmax, concatenation, top-k -- are not in
it) and the sum of kernel time per token from the device-side kernel events of torch.profiler over one more generation
(every kernel, torch's included; null when the profiler is unavailable)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (model type, workload of bench.py, beam, time limit of the leg in seconds)
LEGS = {
    "t-ARK@syn-paths": ("t-ARK", "syn-paths", 1, 120),
    "t-SAIL@syn-paths/beam1": ("t-SAIL", "syn-paths", 1, 120),
    "t-SAIL@syn-paths/beam4": ("t-SAIL", "syn-paths", 4, 120),
    "t-ARK@wd-articles": ("t-ARK", "wd-articles", 1, 240),
    "t-SAIL@wd-articles/beam1": ("t-SAIL", "wd-articles", 1, 240),
    "t-SAIL@wd-articles/beam4": ("t-SAIL", "wd-articles", 4, 300),
}


def run_leg(name, precision, batch, kernel_time):
    import torch
    import bench
    from ark_amd import engine as E
    from kgvae.model.models import ARK, SAIL
    from kgvae.model.utils import seq_to_triples
    mt, wl, beam, _ = LEGS[name]
    cfg = dict(bench.build_cfg(0.0, wl), model_type=mt, precision=precision)
    torch.manual_seed(0)
    model = (ARK if mt == "t-ARK" else SAIL)(cfg).to("cuda")
    model.eval()
    eng = model.engine()
    st, seq_len = cfg["special_tokens"], cfg["seq_len"]
    z = torch.randn(batch, cfg["d_latent"], generator=torch.Generator().manual_seed(1)).cuda()
    steps = {"n": 0}
    def counted(*a, _f=eng.decode_step, **k):
        steps["n"] += 1
        return _f(*a, **k)
    eng.decode_step = counted

    def generate(length):
        if mt == "t-ARK":
            return model.generate(length, st, batch_size=batch)
        return model.decode_latent(z, length, st, seq_to_triples, cfg["ENT_BASE"], cfg["REL_BASE"], beam=beam)

    out = {"model": mt, "workload": wl, "beam": beam, "batch": batch, "seq_len": seq_len, "precision": precision}
    reps = 5 if seq_len <= 64 else 1
    for on in (True, False):
        eng.kv_cache = on
        generate(min(seq_len, 25))            # warm-up: 24 positions (past the 16 at which the prefix path changes kernels)
        torch.cuda.synchronize()
        ms, launches, ntok = [], 0, 0
        for _ in range(reps):
            steps["n"] = 0
            c0 = E._calls[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            generate(seq_len)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ntok = steps["n"]   # generated positions = decode_step calls (the prefix state re-runs its beams inside one)
            launches = (E._calls[0] - c0) / ntok
            ms.append(dt * 1e3 / ntok)
        res = {"ms_per_token": statistics.median(ms), "tokens": ntok, "library_launches_per_token": round(launches, 2), "generations_timed": reps,
               "kernel_ms_per_token": None}
        if kernel_time:
            try:
                from torch.autograd import DeviceType
                from torch.profiler import ProfilerActivity, profile
                steps["n"] = 0
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    generate(seq_len)
                    torch.cuda.synchronize()
                us, nk = 0.0, 0
                for ev in prof.events():
                    if ev.device_type == DeviceType.CUDA:   # device-side events: their own duration
                        us += float(ev.device_time_total)
                        nk += 1
                res["kernel_events_per_token"] = round(nk / steps["n"], 2)
                if nk >= launches * steps["n"]:
                    res["kernel_ms_per_token"] = us / 1e3 / steps["n"]
                else:   # (fewer device events than library launches: the profiler's buffer dropped some -- no figure)
                    res["kernel_time_error"] = "the profiler kept fewer kernel events than the library launched"
            except Exception as e:   # (a figure that could not be taken is reported as missing, never estimated)
                res["kernel_time_error"] = repr(e)[:200]
        out["kv_cache" if on else "prefix_rerun"] = res
    out["speedup"] = out["prefix_rerun"]["ms_per_token"] / out["kv_cache"]["ms_per_token"]
    out["peak_GiB"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="mixed")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--no-kernel-time", action="store_true")
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)   # (child mode: run this one leg in this process)
    args = ap.parse_args()
    if args.leg:
        run_leg(args.leg, args.precision, args.batch, not args.no_kernel_time)
        return 0
    result = {"tool": "decode_bench", "precision": args.precision, "batch": args.batch, "legs": {}}
    rc = 0
    for name in args.legs:
        cmd = ["timeout", "-k", "10", str(LEGS[name][3]), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--precision", args.precision, "--batch", str(args.batch)] + (["--no-kernel-time"] if args.no_kernel_time else [])
        print("[decode_bench]", name, file=sys.stderr, flush=True)
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
